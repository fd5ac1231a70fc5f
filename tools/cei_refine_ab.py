"""Gradient refinement of the constrained pick (robo_cei_refine_cand) against what it is made of, at N = 4096, D = 16,
65 536 device-resident candidates, 256 starts, 50 steps, C = 1, 2 and 4 constraints, LogEI + log PoF.

A  the yardstick, from entry points that predate the call: C + 1 calls of robo_acq_refine_cand (LogEI) on GPs of the same
   shape -- each one sweep, the selection, 51 x (scale, cross-gradient rows, solve, epilogue) -- plus one robo_cei_eval_cand
   without values (the C + 1 sweeps and the fold once more: the sum counts the sweeps twice).  --only-a measures A alone:
   that is how the tool runs on a checkout of the parent commit, which has no B, for the yardstick on the same data.
B  one robo_cei_refine_cand: C + 1 sweeps, the fold, the selection, 51 x (C + 1) x (scale, cross-gradient rows, solve,
   epilogue), one synchronisation.
The expectation, derived from the launch sequences and not measured before this tool: B is close to A minus the C + 1 sweeps
A counts twice and the C selections it repeats, i.e. a little below A.
HIP events on the context's stream; medians (min - max) of --reps repetitions after a warm-up, A and B alternating; one
JSON record (stdout, and --out PATH).  The epilogue's share of B is read from a kernel trace of one B call (rocprofv3
--kernel-trace --stats -- python tools/cei_refine_ab.py --reps 1 --only-b), not from this tool's timers.

    python tools/cei_refine_ab.py [--reps 5] [--only-a | --only-b] [--out cei_refine_ab.json]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robo_amd import _lib  # noqa: E402

N, D, M, K, T = 4096, 16, 65536, 256, 50
CS = (1, 2, 4)
KIND = "log_ei"


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": len(ms)}


def problem(ctx):
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
    return obj, cons, th, _lib.Candidates(ctx, m=M, dim=D, seed=1), float(np.median(y))


def timed(ctx, fn):
    ctx.record(0)
    out = fn()
    ctx.record(1)
    ctx.synchronize()
    return ctx.elapsed_ms(0, 1), out


def yardstick(ctx, obj, cons, th, cand, eta, Cn):
    """-> (ms of the C + 1 plain refinements, ms of the constrained sweep)"""
    ms = 0.0
    for g in [obj] + cons[:Cn]:
        ms += timed(ctx, lambda: g.refine(KIND, 0.0, eta, cand, K, T, 0.05))[0]
    return ms, timed(ctx, lambda: obj.cei(cons[:Cn], cand, th[:Cn], KIND, 0.0, eta, want_values=False))[0]


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    only_a, only_b = "--only-a" in args, "--only-b" in args
    rec = {"N": N, "D": D, "M": M, "K": K, "T": T, "kind": KIND,
           "note": "one run on one machine; A = C + 1 robo_acq_refine_cand + one robo_cei_eval_cand (no values)", "C": {}}
    ctx = _lib.default_context()
    rec["device"] = ctx.name
    obj, cons, th, cand, eta = problem(ctx)
    for Cn in CS:
        a_runs, b_ms, res = [], [], None
        for r in range(reps + 1):
            a = None if only_b else yardstick(ctx, obj, cons, th, cand, eta, Cn)
            if not only_a:
                b, res = timed(ctx, lambda: obj.cei_refine(cons[:Cn], cand, th[:Cn], KIND, 0.0, eta, K, T, 0.05))
            if r >= 1:
                if not only_a:
                    b_ms.append(b)
                if not only_b:
                    a_runs.append(a)
        out = {}
        if b_ms:
            out.update({"B_cei_refine": stats(b_ms), "value": res.value, "flags": res.flags})
        if a_runs:
            total = [x[0] + x[1] for x in a_runs]
            out["A"] = {"refines": stats([x[0] for x in a_runs]), "cei_sweep": stats([x[1] for x in a_runs]),
                        "sum": stats(total)}
            if b_ms:
                out["B_over_A"] = float(np.median(b_ms) / np.median(total))
        rec["C"][str(Cn)] = out
    for h in [cand, obj] + cons:
        h.close()
    line = json.dumps(rec)
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
