"""Parzen estimators on the device (robo_kde_*): what the fused density-ratio sweep costs, next to the same ratio on the host
and to one EI sweep of a GP of the same size.

A  one fused call (robo_kde_ratio_eval_cand, argmax only) of 65 536 candidates through two mixtures of N = 4096 observations
   split at gamma = 0.15 (hyperopt bandwidths, a prior component each), D in {2, 16, 64}: wall clock around the call, which
   ends in its synchronisation (upload, sweep, argmax), and the sweep kernel alone (event slots 30 -> 31).  Two warm-up calls,
   the median of --reps.  Pairs per second count both mixtures: 65 536 x (N + 2).
B  the same ratio on the host: NumPy with SciPy's logsumexp over blocks of 512 candidates, at the BLAS thread count of the
   environment (set OMP_NUM_THREADS=64 for the README's CPU column; the record states what threadpoolctl reports).  Timed on --host-points candidates and
   reported per candidate: nothing is extrapolated.
C  one EI sweep (robo_acq_eval, argmax only) of the same 65 536 candidates over a GP fitted to the same 4096 x 16 observations:
   wall clock; the fused TPE call's share of it.
One JSON record (stdout, and --out PATH).

    python tools/tpe_ab.py [--reps 5] [--host-points 2048] [--out tpe_ab.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robo_amd import _lib  # noqa: E402
from robo_amd.models import tpe as T  # noqa: E402

N, M = 4096, 65536


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": len(ms)}


def host_ratio(mixes, X, block=512):
    from scipy.special import logsumexp, ndtr
    out = []
    for mu, h, w in mixes:
        h = np.broadcast_to(h, mu.shape)
        c = np.log(w / w.sum()) - (np.log(h) + 0.5 * np.log(2 * np.pi) + np.log(ndtr((1 - mu) / h) - ndtr(-mu / h))).sum(axis=1)
        ih2 = 1.0 / (h * h)
        cq = c - 0.5 * (mu * mu * ih2).sum(axis=1)
        lp = np.empty(X.shape[0])
        for r0 in range(0, X.shape[0], block):
            x = X[r0:r0 + block]
            lp[r0:r0 + block] = logsumexp(cq[None] + x @ (mu * ih2).T - 0.5 * (x * x) @ ih2.T, axis=1)
        out.append(lp)
    return out[0] - out[1]


def main():
    args = sys.argv[1:]

    def opt(name, default):
        return int(args[args.index(name) + 1]) if name in args else default
    reps, host_points = opt("--reps", 5), opt("--host-points", 2048)
    ctx = _lib.default_context()
    rec = {"device": ctx.name, "n": N, "m": M, "note": "one run on one machine", "shapes": {}}
    for D in (2, 16, 64):
        rs = np.random.RandomState(D)
        X = rs.rand(N, D)
        y = np.sinc(X * 10 - 5).sum(axis=1) + 0.1 * rs.randn(N)
        mixes = [T.hyperopt_mixture(X[idx]) for idx in T.split(y, 0.15)]
        kde = _lib.DeviceKDE(ctx, np.zeros(D), np.ones(D))
        for which, mix in enumerate(mixes):
            kde.set_mixture(which, *mix)
        Xc, wall, kern = rs.rand(M, D), [], []
        for rep in range(reps + 2):
            t0 = time.perf_counter()
            best = kde.ratio(Xc, want_values=False)[3:]
            dt = 1e3 * (time.perf_counter() - t0)
            if rep >= 2:
                wall.append(dt)
                kern.append(ctx.elapsed_ms(30, 31))
        pairs = float(M) * (N + 2)
        row = {"fused_call": stats(wall), "sweep_kernel": stats(kern), "pairs_per_s_kernel": pairs / (1e-3 * np.median(kern)),
               "argmax": int(best[1])}
        t0 = time.perf_counter()
        ref = host_ratio(mixes, Xc[:host_points])
        row["host"] = {"points": host_points, "ms_per_1000_candidates": 1e6 * (time.perf_counter() - t0) / host_points,
                       "max_abs_diff": float(np.max(np.abs(ref - kde.ratio(Xc[:host_points])[0])))}
        if D == 16:
            from robo_amd.acquisition_functions import EI
            from robo_amd.kernels import Matern52Kernel
            from robo_amd.models import GaussianProcess
            theta = np.concatenate([[0.0], np.full(D, np.log(0.25 * D)), [np.log(1e-3)]])
            model = GaussianProcess(Matern52Kernel(np.exp(theta[1:-1]), ndim=D, log_amp=theta[0]), noise=1e-3, lower=np.zeros(D),
                                    upper=np.ones(D))
            model.train(X, y, do_optimize=False)
            acq, ei = EI(model), []
            for rep in range(reps + 2):
                t0 = time.perf_counter()
                acq.argmax(Xc)
                if rep >= 2:
                    ei.append(1e3 * (time.perf_counter() - t0))
            row["ei_sweep_same_shape"] = stats(ei)
            row["share_of_ei_sweep"] = float(np.median(wall) / np.median(ei))
        rec["shapes"]["D%d" % D] = row
        kde.close()
    try:
        import threadpoolctl
        rec["host_threads"] = [p["num_threads"] for p in threadpoolctl.threadpool_info()]
    except ImportError:
        rec["host_threads"] = "threadpoolctl not importable: the environment's default"
    line = json.dumps(rec)
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
