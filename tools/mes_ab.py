"""Max-value entropy search on the device (robo_mes_eval_cand) against the sweep it rides on, at N = 4096, D = 16,
65 536 device-resident candidates, K = 10, values not copied back.

A  robo_acq_eval_cand, EI: one sweep + the closed-form tail (the baseline; its code path predates MES).
B  robo_mes_eval_cand: the same sweep + bracket, quantile search, Gumbel fit, draws, values, argmax.
   B - A is the tail; the context's phase events split the last call into sweep (24 -> 27), minimum sampling (27 -> 30)
   and element-wise half (30 -> 31).
C  the marginal forms at N = 2048, S = 3: robo_acq_eval_marginal_cand (EI) against robo_mes_eval_marginal_cand.
HIP events on the context's stream; medians (min - max) of --reps repetitions after a warm-up, A and B alternating; one
JSON record (stdout, and --out PATH).

    python tools/mes_ab.py [--reps 7] [--out mes_ab.json]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robo_amd import _lib  # noqa: E402

N, D, M, K = 4096, 16, 65536, 10
N_MARGINAL, S = 2048, 3


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": len(ms)}


def alternate(ctx, legs, reps, warm=2):
    """every repetition times each leg once, in turn"""
    out = {name: [] for name in legs}
    for rep in range(reps + warm):
        for name, fn in legs.items():
            ctx.record(0)
            fn()
            ctx.record(1)
            ctx.synchronize()
            if rep >= warm:
                out[name].append(ctx.elapsed_ms(0, 1))
    return out


def fitted(ctx, n, rs, ls_scale=1.0, noise=1e-3):
    X = rs.rand(n, D)
    y = np.sinc(X * 10 - 5).sum(axis=1)
    g = _lib.DeviceGP(ctx, "matern52", n, D)
    g.set_data(X, y)
    g.fit(np.concatenate([[0.0], np.full(D, np.log(0.25 * D * ls_scale)), [np.log(noise)]]), float(y.mean()))
    return g, float(y.min())


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 7
    ctx = _lib.default_context()
    rs = np.random.RandomState(0)
    u = rs.rand(S, K)
    cand = _lib.Candidates(ctx, m=M, dim=D, seed=1)
    rec = {"device": ctx.name, "N": N, "D": D, "M": M, "K": K, "note": "one run on one machine"}

    g, eta = fitted(ctx, N, rs)
    t = alternate(ctx, {"A": lambda: g.acq("ei", 0.0, eta, cand, want_values=False),
                        "B": lambda: g.mes(eta, cand, u[0], want_values=False)}, reps)
    rec["A_ei"], rec["B_mes"] = stats(t["A"]), stats(t["B"])
    rec["B_minus_A"] = stats([b - a for a, b in zip(t["A"], t["B"])])
    rec["B_over_A"] = rec["B_mes"]["median_ms"] / rec["A_ei"]["median_ms"]
    rec["B_phases_ms"] = {"sweep": ctx.elapsed_ms(24, 27), "minimum_sampling": ctx.elapsed_ms(27, 30),
                          "elementwise": ctx.elapsed_ms(30, 31)}
    g.close()

    gps, etas = [], []
    for s in range(S):
        gs, e = fitted(ctx, N_MARGINAL, np.random.RandomState(5), 0.8 + 0.2 * s, 1e-3 * (1 + s))
        gps.append(gs)
        etas.append(e - 0.01 * s)
    t = alternate(ctx, {"A": lambda: _lib.acq_marginal(gps, "ei", 0.0, np.array(etas), cand, want_values=False),
                        "B": lambda: _lib.mes_marginal(gps, np.array(etas), cand, u, want_values=False)}, reps)
    rec["marginal"] = {"N": N_MARGINAL, "S": S, "A_ei": stats(t["A"]), "B_mes": stats(t["B"]),
                       "B_minus_A": stats([b - a for a, b in zip(t["A"], t["B"])]),
                       "B_over_A": float(np.median(t["B"]) / np.median(t["A"]))}
    for gs in gps:
        gs.close()
    cand.close()
    line = json.dumps(rec)
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
