"""Hyper-parameter optimisation on the device (robo_gp_grad_loglik_batch, robo_gp_optimize_hypers) against what it replaces,
Matern-5/2, D = 16.

A  robo_gp_grad_loglik_batch at S = 8 against 8 sequential robo_gp_grad_loglik calls of the same build, at
   N = 256, 512, 1024, 2048: synchronised host clock around the calls (both legs end synchronised), the legs alternating.
B  GaussianProcess.train(do_optimize=True) with optimizer="host" (the reference's SciPy L-BFGS-B on finite differences, the
   code of the parent commit) and optimizer="device" (8 starts, 60 iterations) at N = 512 and 2048, DefaultPrior: wall time
   and final nll of each, the legs alternating.
Medians (min - max) of --reps repetitions after a warm-up; one JSON record (stdout, and --out PATH).

    python tools/hyperopt_ab.py [--reps 5] [--train-reps 2] [--out hyperopt_ab.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robo_amd import _lib  # noqa: E402

D, S = 16, 8
GRAD_SIZES = (256, 512, 1024, 2048)
TRAIN_SIZES = (512, 2048)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": len(ms)}


def alternate(ctx, legs, reps, warm=1):
    """every repetition times each leg once, in turn; every leg ends synchronised"""
    out = {name: [] for name in legs}
    for rep in range(reps + warm):
        for name, fn in legs.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            if rep >= warm:
                out[name].append(1e3 * (time.perf_counter() - t0))
    return out


def data(n, rs):
    X = rs.rand(n, D)
    return X, np.sin(3 * X.sum(axis=1) / np.sqrt(D / 3.0)) + 0.1 * rs.randn(n)


def grad_leg(ctx, n, reps):
    rs = np.random.RandomState(n)
    X, y = data(n, rs)
    g = _lib.DeviceGP(ctx, "matern52", n, D)
    g.set_data(X, y)
    base = np.concatenate([[0.0], np.full(D, np.log(0.3 * D)), [np.log(1e-2)]])
    thetas = base[None, :] + 0.3 * rs.randn(S, base.size)
    mean_c = float(y.mean())
    ll, grad, st = g.grad_loglik_batch(thetas, mean_c)
    same = all(np.array_equal(grad[s], g.grad_loglik(thetas[s], mean_c)[1]) for s in range(S))
    t = alternate(ctx, {"sequential": lambda: [g.grad_loglik(th, mean_c) for th in thetas],
                        "batched": lambda: g.grad_loglik_batch(thetas, mean_c)}, reps)
    g.close()
    rec = {k: stats(v) for k, v in t.items()}
    rec["same_bits"] = bool(same and np.all(st == 0))
    rec["batched_over_sequential"] = rec["batched"]["median_ms"] / rec["sequential"]["median_ms"]
    return rec


def train_leg(n, reps):
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models import GaussianProcess
    from robo_amd.priors import DefaultPrior
    X, y = data(n, np.random.RandomState(n + 1))
    rec = {"host": {"ms": [], "nll": []}, "device": {"ms": [], "nll": []}}
    for rep in range(reps + 1):
        for opt in ("host", "device"):
            kernel = (2.0 * D) * Matern52Kernel(np.ones(D), ndim=D)
            prior = DefaultPrior(len(kernel) + 1, rng=np.random.RandomState(0))
            m = GaussianProcess(kernel, prior=prior, lower=np.zeros(D), upper=np.ones(D), rng=np.random.RandomState(1),
                                optimizer=opt)
            t0 = time.perf_counter()
            m.train(X, y, do_optimize=True)
            ms = 1e3 * (time.perf_counter() - t0)
            if rep >= 1 or reps == 0:
                rec[opt]["ms"].append(ms)
                rec[opt]["nll"].append(float(m.nll(m.hypers)))
            m.gp.close()
    return {opt: dict(stats(r["ms"]), nll=r["nll"][0]) for opt, r in rec.items()}


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    train_reps = int(args[args.index("--train-reps") + 1]) if "--train-reps" in args else 2
    ctx = _lib.default_context()
    out = {"device": ctx.name, "D": D, "S": S, "grad": {}, "train": {}}
    for n in GRAD_SIZES:
        out["grad"][str(n)] = grad_leg(ctx, n, reps)
        print("grad N=%d: %s" % (n, json.dumps(out["grad"][str(n)])), file=sys.stderr, flush=True)
    for n in TRAIN_SIZES:
        out["train"][str(n)] = train_leg(n, train_reps)
        print("train N=%d: %s" % (n, json.dumps(out["train"][str(n)])), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if "--out" in args:
        path = args[args.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
