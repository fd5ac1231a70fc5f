"""Two-objective expected hypervolume improvement on the device (robo_ehvi_eval_cand) against the two sweeps it rides on,
at N = 4096, D = 16, 65 536 device-resident candidates, fronts of P = 16, 64, 256 and 1024 points, values not copied back.

A  two robo_acq_eval_cand calls, EI, one per GP: two sweeps + two closed-form tails (the yardstick; its code path predates
   EHVI).  The acquisition screen of argmax-only calls is switched off (acq_screen = 0) for the whole run, so that A solves
   every candidate as B has to.
B  robo_ehvi_eval_cand per P: the same two sweeps + two copies of the moments + the strip kernel + argmax, one
   synchronisation.  The strip kernel from the context's phase events (30 -> 31).
HIP events on the context's stream; medians (min - max) of --reps repetitions after a warm-up, A and B alternating; one
JSON record (stdout, and --out PATH).

    python tools/ehvi_ab.py [--reps 7] [--out ehvi_ab.json]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robo_amd import _lib  # noqa: E402

N, D, M = 4096, 16, 65536
PS = (16, 64, 256, 1024)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": len(ms)}


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 7
    ctx = _lib.default_context()
    ctx.set_tuning("acq_screen", 0)
    rs = np.random.RandomState(0)
    X = rs.rand(N, D)
    ys = (np.sinc(X * 10 - 5).sum(axis=1), np.cos(3 * X).sum(axis=1) + 0.1 * rs.randn(N))
    gps = []
    for kind, y, ls2 in zip(("matern52", "rbf"), ys, (0.25 * D, 0.4 * D)):
        g = _lib.DeviceGP(ctx, kind, N, D)
        g.set_data(X, y)
        g.fit(np.concatenate([[0.0], np.full(D, np.log(ls2)), [np.log(1e-3)]]), float(y.mean()))
        gps.append(g)
    cand = _lib.Candidates(ctx, m=M, dim=D, seed=1)
    lo = np.array([ys[0].min(), ys[1].min()])
    ref = np.array([ys[0].max(), ys[1].max()]) + 0.1
    rec = {"device": ctx.name, "N": N, "D": D, "M": M, "note": "one run on one machine; acq_screen = 0", "P": {}}
    for P in PS:
        t = np.sort(rs.rand(P))
        front = lo + np.stack((t, 1.0 - np.sqrt(t)), axis=1) * (ref - 0.05 - lo)
        a_ms, b_ms, k_ms = [], [], []
        for r in range(reps + 2):
            ctx.record(0)
            for g, y in zip(gps, ys):
                g.acq("ei", 0.0, float(y.min()), cand, want_values=False)
            ctx.record(1)
            ctx.synchronize()
            a = ctx.elapsed_ms(0, 1)
            ctx.record(0)
            res = gps[0].ehvi(gps[1], cand, front, ref, want_values=False)
            ctx.record(1)
            ctx.synchronize()
            if r >= 2:
                a_ms.append(a)
                b_ms.append(ctx.elapsed_ms(0, 1))
                k_ms.append(ctx.elapsed_ms(30, 31))
        rec["P"][str(P)] = {"A_two_ei": stats(a_ms), "B_ehvi": stats(b_ms), "strip_kernel": stats(k_ms),
                            "chunk": cand.chunk(), "max": res.max, "flags": res.flags,
                            "kernel_share_of_call": float(np.median(k_ms) / np.median(b_ms)),
                            "B_over_A": float(np.median(b_ms) / np.median(a_ms))}
    cand.close()
    for g in gps:
        g.close()
    ctx.set_tuning("acq_screen", None)
    line = json.dumps(rec)
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
