"""Host vs device EP for p_min (robo_amd/util/epmgp.py joint_min vs joint_min_device / joint_min_batch), device-synchronised
wall clock after warm-up, and one MarginalizationGPMCMC.update of the default entropy_search wiring (gp_mcmc, Branin) with
each backend.  Writes one JSON record (stdout, and --out PATH).  Kernel times: run this under
`rocprofv3 --kernel-trace --stats -- python tools/ep_ab.py --quick`.

    python tools/ep_ab.py [--reps 7] [--quick] [--out ep_ab.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robo_amd import _lib  # noqa: E402
from robo_amd.util import epmgp  # noqa: E402


def belief(nb, rs):
    """a random RBF belief over nb points in 2-d (the shape of the issue's host measurement)"""
    Z = rs.rand(nb, 2)
    d2 = ((Z[:, None, :] - Z[None, :, :]) ** 2).sum(-1)
    return rs.randn(nb) * 0.3, np.exp(-0.5 * d2 / 0.3 ** 2) + 1e-6 * np.eye(nb)


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()                                  # the device entry points return after the stream has synchronised
        out.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * float(np.median(out)), "min_ms": 1e3 * min(out), "max_ms": 1e3 * max(out), "reps": reps}


def branin(x):
    x = np.asarray(x).ravel()
    return float((x[1] - 5.1 / (4 * np.pi ** 2) * x[0] ** 2 + 5 / np.pi * x[0] - 6) ** 2 +
                 10 * (1 - 1 / (8 * np.pi)) * np.cos(x[0]) + 10)


def marginal_update(reps):
    from robo_amd.fmin.entropy_search import build_entropy_search
    lo, hi = np.array([-5.0, 0.0]), np.array([10.0, 15.0])
    rs = np.random.RandomState(0)
    gp, acq, _ = build_entropy_search(lo, hi, "random", "gp_mcmc", rs)
    X = lo + (hi - lo) * rs.rand(10, 2)
    gp.train(X, np.array([branin(x) for x in X]), do_optimize=True)
    out = {"n_estimators": len(gp.models)}
    for backend in ("host", "device"):
        acq.acquisition_func.ep = backend
        for e in acq.estimators:
            e.ep = backend
        out[backend] = timed(lambda: acq.update(gp), reps)
    return out


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 7
    quick = "--quick" in args
    ctx = _lib.default_context()
    rs = np.random.RandomState(1)
    rec = {"device": ctx.name, "per_call": {}, "batch": {}}
    for nb in (50, 64):
        mu, var = belief(nb, rs)
        host = timed(lambda: epmgp.joint_min(mu, var, with_derivatives=True), 1 if quick else 3)
        dev = timed(lambda: epmgp.joint_min_device(mu, var, with_derivatives=True, ctx=ctx), reps)
        rec["per_call"]["nb%d" % nb] = {"host": host, "device": dev, "speedup": host["median_ms"] / dev["median_ms"]}
    for S in (12, 54):
        bs = [belief(50, rs) for _ in range(S)]
        mus, vars_ = np.array([b[0] for b in bs]), np.array([b[1] for b in bs])
        rec["batch"]["S%d_nb50" % S] = timed(lambda: epmgp.joint_min_batch(mus, vars_, True, ctx=ctx), reps)
    if not quick:
        rec["marginal_update_entropy_search_gp_mcmc"] = marginal_update(3)
    line = json.dumps(rec)
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
