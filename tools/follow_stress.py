"""Hand-off stress: fits in the follower form (single-theta step kernel and the batched merged launch) while ANOTHER context
of the same device keeps the chip busy with large posterior evaluations (uneven load, other kernels in the CUs' L1 / L2) --
every word of every factor and every likelihood must equal the launch-per-phase reference, iteration after iteration.
The reference itself (single-theta likelihood and every sample of the batch) is anchored on the fp64 oracle first, and
every mismatch names the side that left the oracle: REFERENCE or FOLLOWER.

    python tools/follow_stress.py [iterations]
"""
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _tol import LOGLIK_RTOL  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402
from robo_amd import _lib  # noqa: E402

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 150
ctx, ctx2 = _lib.Context(0), _lib.Context(0)
stop = threading.Event()


def background():
    N, D, M = 2048, 8, 32768
    rs = np.random.RandomState(9)
    X = rs.rand(N, D)
    y = np.sin(X.sum(axis=1))
    th = np.concatenate([[0.0], np.full(D, np.log(0.25 * D)), [np.log(1e-3)]])
    g = _lib.DeviceGP(ctx2, "matern52", N, D)
    g.set_data(X, y)
    g.fit(th, 0.0)
    cand = _lib.Candidates(ctx2, rs.rand(M, D))
    n = 0
    while not stop.is_set():
        g.acq("ei", 0.0, float(y.min()), cand, want_values=False)
        n += 1
    background.count = n


def oracle_loglik(X, y, theta):
    return O.gp_log_likelihood(O.gp_compute("matern52", theta, X), y, 0.0)


def off_oracle(ll, ll_o):
    return not abs(ll - ll_o) <= LOGLIK_RTOL * abs(ll_o)


bad = 0
t = threading.Thread(target=background)
t.start()
try:
    for N, D in ((4096, 16), (1500, 6), (700, 3)):
        rs = np.random.RandomState(N)
        X = rs.rand(N, D)
        y = np.sinc(X * 10 - 5).sum(axis=1)
        th = np.concatenate([[0.0], np.full(D, np.log(0.25 * D)), [np.log(1e-3)]])
        g = _lib.DeviceGP(ctx, "matern52", N, D)
        g.set_data(X, y)
        S = 12
        thetas = th[None, :] + 0.1 * rs.randn(S, th.size)
        ctx.set_tuning("potrf_follow", 0)
        g.fit(th, 0.0)                       # warm-up: the handle's first fit and first batch are not the reference
        ll0 = g.fit(th, 0.0)
        L0 = g.factor().copy()
        ctx.set_tuning("potrf_follow", None)
        ctx.set_tuning("potrf_batch_follow", 0)
        g.loglik_batch(thetas, 0.0)
        b0, _ = g.loglik_batch(thetas, 0.0)
        # the reference against the fp64 oracle (mean 0, as the fits above)
        ll_o = oracle_loglik(X, y, th)
        b_o = np.array([oracle_loglik(X, y, tt) for tt in thetas])
        if off_oracle(ll0, ll_o):
            bad += 1
            print("REFERENCE single N=%d off the oracle: ll0 - oracle = %g" % (N, ll0 - ll_o), flush=True)
        for s in range(S):
            if off_oracle(b0[s], b_o[s]):
                bad += 1
                print("REFERENCE batched N=%d sample %d off the oracle: b0 - oracle = %g" % (N, s, b0[s] - b_o[s]), flush=True)
        t0 = time.perf_counter()
        for it in range(ITERS):
            ctx.set_tuning("potrf_follow_rows", (64, 128, -1)[it % 3])
            ll = g.fit(th, 0.0)
            L = g.factor() if it % 10 == 0 else None
            if ll != ll0 or (L is not None and not np.array_equal(L, L0)):
                bad += 1
                print("MISMATCH single N=%d it=%d  dll=%g  %s  (follower - oracle %g, reference - oracle %g)" % (
                    N, it, ll - ll0, "FOLLOWER" if off_oracle(ll, ll_o) else "REFERENCE" if off_oracle(ll0, ll_o) else
                    "both within the oracle's tolerance", ll - ll_o, ll0 - ll_o), flush=True)
            ctx.set_tuning("potrf_batch_follow", 1)
            ctx.set_tuning("potrf_batch_roll", it & 1)
            b, st = g.loglik_batch(thetas, 0.0)
            if not np.array_equal(b, b0):
                bad += 1
                for s in np.nonzero(b != b0)[0]:
                    print("MISMATCH batched N=%d it=%d sample %d  d=%g  %s  (follower - oracle %g, reference - oracle %g)" % (
                        N, it, s, b[s] - b0[s], "FOLLOWER" if off_oracle(b[s], b_o[s]) else
                        "REFERENCE" if off_oracle(b0[s], b_o[s]) else "both within the oracle's tolerance",
                        b[s] - b_o[s], b0[s] - b_o[s]), flush=True)
        for k in ("potrf_follow_rows", "potrf_batch_follow", "potrf_batch_roll"):
            ctx.set_tuning(k, None)
        print("N=%d: %d iterations (single-theta follower fit + batched merged launch, %d thetas) under load: %s  (%.1f s)" % (
            N, ITERS, S, "all bit-identical" if bad == 0 else "%d MISMATCHES" % bad, time.perf_counter() - t0), flush=True)
        g.close()
finally:
    stop.set()
    t.join()
print("background posterior evaluations meanwhile:", getattr(background, "count", None))
sys.exit(1 if bad else 0)
