"""Joint Monte-Carlo batch EI on the device (robo_qei_batch_cand) against the fantasised greedy selection
(robo_acq_batch_cand, kriging believer), at N = 4096, D = 16, 65 536 device-resident candidates, q = 8, K = 128 and 512.

A  robo_qei_batch_cand with q = 8 for every K, and with q = 1 (= one sweep): HIP events on the context's stream.
   (A(q = 8) - A(q = 1)) / 7 is the cost of a pick after the first.  The library's event slots 30 -> 31 bracket the
   fold kernel of the LAST pick (j = 7: the deepest history): its share of a later pick.
B  robo_acq_batch_cand (kriging believer), same q, in the same session, the two alternating.
Every (q, K) of A runs on a GP handle of its own (the same data and theta), so each keeps its state block between the
repetitions as B does: no timed call allocates.
Medians (min - max) of --reps repetitions after a warm-up; one JSON record (stdout, and --out PATH).  Kernel shares: run
under `rocprofv3 --kernel-trace --stats -- python tools/qei_ab.py --reps 3`.

    python tools/qei_ab.py [--reps 5] [--out qei_ab.json]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robo_amd import _lib  # noqa: E402

N, D, M, Q = 4096, 16, 65536, 8
KS = (128, 512)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": len(ms)}


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    ctx = _lib.default_context()
    rs = np.random.RandomState(0)
    X = rs.rand(N, D)
    y = np.sinc(X * 10 - 5).sum(axis=1)
    theta = np.concatenate([[0.0], np.full(D, np.log(0.25 * D)), [np.log(1e-3)]])
    def fitted():
        h = _lib.DeviceGP(ctx, "matern52", N, D)
        h.set_data(X, y)
        h.fit(theta, float(y.mean()))
        return h

    g = fitted()                                  # q = 1 and the believer (their states are separate blocks)
    gk = {K: fitted() for K in KS}
    eta = float(y.min())
    cand = _lib.Candidates(ctx, m=M, dim=D, seed=1)
    rec = {"device": ctx.name, "N": N, "D": D, "M": M, "q": Q, "acq": "ei", "note": "one run on one machine"}

    def timed(fn):
        ctx.record(0)
        r = fn()
        ctx.record(1)
        ctx.synchronize()
        return r, ctx.elapsed_ms(0, 1)

    legs = {"q1": [], "believer": []}
    legs.update({("joint", K): [] for K in KS})
    folds = {K: [] for K in KS}
    picks = {}
    for rep in range(reps + 2):                   # the legs alternate: every repetition yields its own differences
        keep = rep >= 2
        _, t = timed(lambda: g.select_batch_joint(0.0, eta, cand, 1, np.zeros((1, 1))))
        if keep:
            legs["q1"].append(t)
        r, t = timed(lambda: g.select_batch("ei", 0.0, eta, cand, Q))
        picks["believer"] = [int(i) for i in r.indices]
        if keep:
            legs["believer"].append(t)
        for K in KS:
            z = np.random.RandomState(K).standard_normal((K, Q))
            r, t = timed(lambda: gk[K].select_batch_joint(0.0, eta, cand, Q, z))
            picks["joint_K%d" % K] = [int(i) for i in r.indices]
            rec["qei_K%d" % K] = float(r.qei[-1])
            if keep:
                legs[("joint", K)].append(t)
                folds[K].append(ctx.elapsed_ms(30, 31))
    rec["A_q1"], rec["B_believer_q8"] = stats(legs["q1"]), stats(legs["believer"])
    rec["B_per_later_pick"] = stats([(b - a) / (Q - 1) for a, b in zip(legs["q1"], legs["believer"])])
    for K in KS:
        rec["A_joint_q8_K%d" % K] = stats(legs[("joint", K)])
        rec["A_per_later_pick_K%d" % K] = stats([(b - a) / (Q - 1) for a, b in zip(legs["q1"], legs[("joint", K)])])
        rec["A_last_fold_kernel_K%d" % K] = stats(folds[K])
        rec["A_over_B_K%d" % K] = rec["A_joint_q8_K%d" % K]["median_ms"] / rec["B_believer_q8"]["median_ms"]
        rec["fold_share_of_a_later_pick_K%d" % K] = rec["A_last_fold_kernel_K%d" % K]["median_ms"] / \
            rec["A_per_later_pick_K%d" % K]["median_ms"]
    rec["picks"] = picks
    cand.close()
    for h in [g] + list(gk.values()):
        h.close()
    line = json.dumps(rec)
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
