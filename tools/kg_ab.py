"""Knowledge gradient on the device (robo_kg_eval_cand) against the sweep it rides on, at N = 4096, D = 16, 65 536
device-resident candidates, nb = 16, 50 and 64 discretisation points, values not copied back.

A  robo_acq_eval_cand, EI: one sweep + the closed-form tail (the yardstick; its code path predates the knowledge gradient).
B  robo_kg_eval_cand per nb: the same sweep + signed cross-covariance per chunk + envelope kernel + argmax; the
   discretisation's solve is cached after the first (warm-up) call.
   Split of B: the envelope kernel from the context's phase events (30 -> 31), the sweep as A's time, the
   cross-covariance as the remainder B - A - kernel (it also holds the nb-double copy of the discretisation's means).
HIP events on the context's stream; medians (min - max) of --reps repetitions after a warm-up, A and B alternating; one
JSON record (stdout, and --out PATH).

    python tools/kg_ab.py [--reps 7] [--out kg_ab.json]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robo_amd import _lib  # noqa: E402

N, D, M = 4096, 16, 65536
NBS = (16, 50, 64)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": len(ms)}


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 7
    ctx = _lib.default_context()
    rs = np.random.RandomState(0)
    X = rs.rand(N, D)
    y = np.sinc(X * 10 - 5).sum(axis=1)
    g = _lib.DeviceGP(ctx, "matern52", N, D)
    g.set_data(X, y)
    noise = 1e-3
    g.fit(np.concatenate([[0.0], np.full(D, np.log(0.25 * D)), [np.log(noise)]]), float(y.mean()))
    cand = _lib.Candidates(ctx, m=M, dim=D, seed=1)
    rec = {"device": ctx.name, "N": N, "D": D, "M": M, "note": "one run on one machine", "nb": {}}
    for nb in NBS:
        rep = _lib.Candidates(ctx, rs.rand(nb, D))
        a_ms, b_ms, k_ms = [], [], []
        for r in range(reps + 2):
            ctx.record(0)
            g.acq("ei", 0.0, float(y.min()), cand, want_values=False)
            ctx.record(1)
            ctx.synchronize()
            a = ctx.elapsed_ms(0, 1)
            ctx.record(0)
            g.kg(cand, rep, noise, True, want_values=False)
            ctx.record(1)
            ctx.synchronize()
            if r >= 2:
                a_ms.append(a)
                b_ms.append(ctx.elapsed_ms(0, 1))
                k_ms.append(ctx.elapsed_ms(30, 31))
        cc = [b - a - k for a, b, k in zip(a_ms, b_ms, k_ms)]
        rec["nb"][str(nb)] = {"A_ei": stats(a_ms), "B_kg": stats(b_ms), "kg_kernel": stats(k_ms),
                              "cross_cov_remainder": stats(cc), "chunk": cand.chunk(),
                              "kernel_share_of_call": float(np.median(k_ms) / np.median(b_ms)),
                              "B_over_A": float(np.median(b_ms) / np.median(a_ms))}
        rep.close()
    cand.close()
    g.close()
    line = json.dumps(rec)
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
