"""Gradient refinement on the device (robo_acq_refine_cand) against what the library offered before it, at N = 4096,
D = 16, LogEI, 65 536 device-resident candidates, K = 64 / 256 / 1024 starts and T = 50 steps.

A  the new call: T = 0 (sweep + selection) and T = 50 (sweep + selection + refinement), alternating; the difference of each
   pair is the refinement alone (median, min, max over the pairs), divided by the 51 evaluation passes the time per
   iteration.  HIP events on the context's stream around the call.
B  the same iterations as a Python loop over robo_gp_predict_grad with the LogEI gradient and the step rule in NumPy on the
   host (what a user could write before): wall clock, every call synchronises.  --scipy: SciPyOptimizer with
   n_restarts = 64 (finite differences, one 1 x D call per value): wall clock, once.
Medians (min - max) of --reps repetitions after a warm-up; one JSON record (stdout, and --out PATH).  Kernel shares: run
under `rocprofv3 --kernel-trace --stats -- python tools/refine_ab.py --reps 3 --only-a --k 256`.

    python tools/refine_ab.py [--reps 20] [--loop-reps 3] [--scipy] [--only-a] [--k 256] [--out refine_ab.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import refine_oracle as RO  # noqa: E402
from robo_amd import _lib  # noqa: E402

N, D, M, T, STEP0 = 4096, 16, 65536, 50, 0.05


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": len(ms)}


def events(ctx, fn, reps, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        ctx.record(0)
        fn()
        ctx.record(1)
        ctx.synchronize()
        out.append(ctx.elapsed_ms(0, 1))
    return stats(out)


def host_loop(g, X0, eta, steps):
    """the algorithm of robo_acq_refine_cand from the starts X0 with robo_gp_predict_grad and NumPy on the host"""
    def fn(X):
        m, v, dm, dv = g.predict_grad(X)
        return RO.acq_value_grad("log_ei", 0.0, eta, m, v, dm, dv)
    X = X0.copy()
    f, gr = fn(X)
    alpha = np.full(len(X), STEP0)
    for _ in range(steps):
        gp = np.where(((X <= 0) & (gr < 0)) | ((X >= 1) & (gr > 0)), 0.0, gr)
        nrm = np.sqrt((gp * gp).sum(axis=1))
        ok = nrm > 0
        Y = np.where(ok[:, None], np.clip(X + alpha[:, None] * gp / np.where(ok, nrm, 1.0)[:, None], 0.0, 1.0), X)
        fy, gy = fn(Y)
        acc = ok & (fy > f)
        X[acc], f[acc], gr[acc] = Y[acc], fy[acc], gy[acc]
        alpha = np.where(acc, np.minimum(2 * alpha, 0.5), alpha / 2)
    return f.max()


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 20
    loop_reps = int(args[args.index("--loop-reps") + 1]) if "--loop-reps" in args else 3
    ctx = _lib.default_context()
    rs = np.random.RandomState(0)
    X = rs.rand(N, D)
    y = np.sinc(X * 10 - 5).sum(axis=1)
    theta = np.concatenate([[0.0], np.full(D, np.log(0.25 * D)), [np.log(1e-3)]])
    g = _lib.DeviceGP(ctx, "matern52", N, D)
    g.set_data(X, y)
    g.fit(theta, float(y.mean()))
    eta = float(y.min())
    cand = _lib.Candidates(ctx, m=M, dim=D, seed=1)
    rec = {"device": ctx.name, "N": N, "D": D, "M": M, "T": T, "acq": "log_ei", "note": "one run on one machine"}
    rec["sweep_only"] = events(ctx, lambda: g.acq("log_ei", 0.0, eta, cand, want_values=False), reps)
    ks = [int(args[args.index("--k") + 1])] if "--k" in args else [64, 256, 1024]
    for K in ks:
        # the two legs alternate, so that every repetition yields its own difference (both are warm: the explicit inverse
        # of the factor is built by the first T > 0 call)
        legs = {0: [], T: []}
        for rep in range(reps + 2):
            for steps in (0, T):
                ctx.record(0)
                g.refine("log_ei", 0.0, eta, cand, K, steps, STEP0)
                ctx.record(1)
                ctx.synchronize()
                if rep >= 2:
                    legs[steps].append(ctx.elapsed_ms(0, 1))
        a0, a1 = stats(legs[0]), stats(legs[T])
        only = stats([b - a for a, b in zip(legs[0], legs[T])])
        r = g.refine("log_ei", 0.0, eta, cand, K, T, STEP0, diagnostics=True)
        one = {"A_sweep_select": a0, "A_sweep_select_refine": a1, "A_refine_only": only,
               "A_refine_only_ms": only["median_ms"],
               "A_ms_per_iteration": only["median_ms"] / (T + 1),
               "solve_gflop_per_iteration": K * (D + 1) * float(N) * N / 1e9,
               "value": r.value, "sweep_value": float(g.acq("log_ei", 0.0, eta, cand, want_values=False)[1]),
               "accepted_steps": int((r.trace[1:, :, -1] == 1).sum()), "flags": r.flags}
        if "--only-a" not in args:
            X0 = cand.points()[r.starts]
            t = []
            for _ in range(loop_reps + 1):
                t0 = time.perf_counter()
                fb = host_loop(g, X0, eta, T)
                t.append(1e3 * (time.perf_counter() - t0))
            one["B_predict_grad_loop"] = stats(t[1:])
            one["B_value"] = float(fb)
            one["B_over_A"] = float(np.median(t[1:])) / one["A_refine_only_ms"]
        rec["K%d" % K] = one
    if "--scipy" in args:
        from robo_amd.acquisition_functions import LogEI
        from robo_amd.kernels import Matern52Kernel
        from robo_amd.maximizers import SciPyOptimizer
        from robo_amd.models import GaussianProcess
        model = GaussianProcess(Matern52Kernel(np.exp(theta[1:-1]), ndim=D, log_amp=theta[0]), noise=1e-3,
                                lower=np.zeros(D), upper=np.ones(D))
        model.train(X, y, do_optimize=False)
        acq = LogEI(model)
        np.random.seed(0)
        t0 = time.perf_counter()
        xs = SciPyOptimizer(acq, np.zeros(D), np.ones(D), n_restarts=64).maximize()
        rec["B_scipy_64_restarts"] = {"wall_ms": 1e3 * (time.perf_counter() - t0), "value": float(acq.compute(xs[None, :])[0])}
    cand.close()
    g.close()
    line = json.dumps(rec)
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
