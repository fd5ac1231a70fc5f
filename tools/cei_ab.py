"""Constrained expected improvement on the device (robo_cei_eval_cand) against the sweep it rides on, at N = 4096, D = 16,
65 536 device-resident candidates, C = 1, 2 and 4 constraints, values copied back in both.

A  one robo_acq_eval_cand call, EI, on the objective's GP with the values requested -- a call that asks for the values is
   never screened, so it solves every candidate: one sweep + the closed-form tail (the yardstick; its code path predates
   the constrained call).
B  robo_cei_eval_cand per C, EI weighted by the probability of feasibility: C + 1 sweeps + their copies into the sample
   tables + the fold kernel + argmax, one synchronisation.  The fold kernel from the context's phase events (32 -> 33).
The expectation to confirm or refute: B is about C + 1 times A, the fold kernel well under 1 % of B (it moves
(2 (C + 1) + 1) * 8 bytes per candidate).
HIP events on the context's stream; medians (min - max) of --reps repetitions after a warm-up, A and B alternating; one
JSON record (stdout, and --out PATH).

    python tools/cei_ab.py [--reps 7] [--out cei_ab.json]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robo_amd import _lib  # noqa: E402

N, D, M = 4096, 16, 65536
CS = (1, 2, 4)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": len(ms)}


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 7
    ctx = _lib.default_context()
    rs = np.random.RandomState(0)
    X = rs.rand(N, D)
    y = np.sinc(X * 10 - 5).sum(axis=1)
    theta = lambda ls2: np.concatenate([[0.0], np.full(D, np.log(ls2)), [np.log(1e-3)]])                # noqa: E731
    obj = _lib.DeviceGP(ctx, "matern52", N, D)
    obj.set_data(X, y)
    obj.fit(theta(0.25 * D), float(y.mean()))
    cons, th = [], []
    for k in range(max(CS)):
        c = np.cos((3 + k) * X).sum(axis=1) + 0.1 * rs.randn(N)
        g = _lib.DeviceGP(ctx, "rbf", N, D)
        g.set_data(X, c)
        g.fit(theta(0.4 * D), float(c.mean()))
        cons.append(g)
        th.append(float(np.median(c)))
    cand = _lib.Candidates(ctx, m=M, dim=D, seed=1)
    eta = float(np.median(y))
    rec = {"device": ctx.name, "N": N, "D": D, "M": M,
           "note": "one run on one machine; values requested in A and B (A is then never screened)", "C": {}}
    for Cn in CS:
        a_ms, b_ms, k_ms = [], [], []
        for r in range(reps + 2):
            ctx.record(0)
            obj.acq("ei", 0.0, eta, cand, want_values=True)
            ctx.record(1)
            ctx.synchronize()
            a = ctx.elapsed_ms(0, 1)
            ctx.record(0)
            res = obj.cei(cons[:Cn], cand, th[:Cn], "ei", 0.0, eta, want_values=True)
            ctx.record(1)
            ctx.synchronize()
            if r >= 2:
                a_ms.append(a)
                b_ms.append(ctx.elapsed_ms(0, 1))
                k_ms.append(ctx.elapsed_ms(32, 33))
        rec["C"][str(Cn)] = {"A_one_ei": stats(a_ms), "B_cei": stats(b_ms), "fold_kernel": stats(k_ms),
                             "chunk": cand.chunk(), "max": res.max, "flags": res.flags,
                             "fold_bytes_per_candidate": (2 * (Cn + 1) + 1) * 8,
                             "kernel_share_of_call": float(np.median(k_ms) / np.median(b_ms)),
                             "B_over_A": float(np.median(b_ms) / np.median(a_ms)),
                             "B_over_A_per_sweep": float(np.median(b_ms) / np.median(a_ms) / (Cn + 1))}
    cand.close()
    for g in [obj] + cons:
        g.close()
    line = json.dumps(rec)
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
