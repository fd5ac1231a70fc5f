"""The regression forest on the device (robo_rf_*): what a fit and a fused sweep cost, next to the reference's pattern on the host.

A  robo_rf_fit at n in {256, 1024, 4096}, D in {2, 16, 64}, T = 30 trees with bootstrapping: wall clock around the call, which
   ends in its synchronisation (upload, presort, all trees).  The same at T = 120 for n = 1024, D = 16: one workgroup grows a
   tree, so the time should not move while T stays below the number of compute units.  Nodes and depth of the trees alongside.
B  one fused sweep (robo_rf_acq_eval_cand, EI, argmax only) of 65 536 candidates through the n = 1024, D = 16 forest: HIP
   events on the context's stream.
C  the reference's pattern on the host over the same node tables: a Python walk per candidate and tree (random_forest.py's
   predict is a loop over points), then one acq_from_moments call per point.  Timed on --host-points candidates and reported
   per point: nothing is extrapolated.
One JSON record (stdout, and --out PATH).  The split between the presort and the grow kernel: run
`rocprofv3 --kernel-trace --stats -- python tools/forest_ab.py --only-fit --reps 3` on its own.

    python tools/forest_ab.py [--reps 5] [--host-points 256] [--only-fit] [--out forest_ab.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robo_amd import _lib  # noqa: E402

T, M = 30, 65536


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": len(ms)}


def data(n, D):
    rs = np.random.RandomState(n + D)
    X = rs.rand(n, D)
    return X, np.sinc(X * 10 - 5).sum(axis=1) + 0.1 * rs.randn(n)


def timed_fit(ctx, n, D, trees, reps):
    X, y = data(n, D)
    rf = _lib.DeviceForest(ctx, D, trees)
    ms = []
    for rep in range(reps + 1):                  # the first fit allocates and loads the code objects
        t0 = time.perf_counter()
        rf.fit(X, y, seed=rep)
        ms.append(1e3 * (time.perf_counter() - t0))
    tr = rf.trees
    out = dict(stats(ms[1:]), nodes_median=float(np.median([len(t) for t in tr])), depth_max=int(max(t["depth"].max() for t in tr)))
    return rf, X, y, out


def host_walk(trees, x):
    mu = np.empty(len(trees))
    var = np.empty(len(trees))
    for t, tr in enumerate(trees):
        i = 0
        while tr["feature"][i] >= 0:
            i = tr["left"][i] if x[tr["feature"][i]] <= tr["threshold"][i] else tr["right"][i]
        mu[t], var[t] = tr["mean"][i], tr["var"][i]
    return mu.mean(), var.mean() + mu.var()


def main():
    args = sys.argv[1:]

    def opt(name, default):
        return int(args[args.index(name) + 1]) if name in args else default
    reps, host_points = opt("--reps", 5), opt("--host-points", 256)
    ctx = _lib.default_context()
    rec = {"device": ctx.name, "trees": T, "note": "one run on one machine", "fit": {}}
    for n in (256, 1024, 4096):
        for D in (2, 16, 64):
            rf, _, _, rec["fit"]["n%d_D%d" % (n, D)] = timed_fit(ctx, n, D, T, reps)
            rf.close()
    rf, _, _, rec["fit"]["n1024_D16_T120"] = timed_fit(ctx, 1024, 16, 120, reps)
    rf.close()
    if "--only-fit" not in args:
        rf, X, y, _ = timed_fit(ctx, 1024, 16, T, 1)
        Xc, eta, ms = np.random.RandomState(1).rand(M, 16), float(y.min()), []
        for rep in range(reps + 2):
            ctx.record(0)
            best = rf.acq("ei", 0.0, eta, Xc, want_values=False)[1:]
            ctx.record(1)
            ctx.synchronize()
            if rep >= 2:
                ms.append(ctx.elapsed_ms(0, 1))
        rec["sweep_65536_n1024_D16"] = dict(stats(ms), argmax=int(best[1]))
        trees = rf.trees
        t0 = time.perf_counter()
        moments = [host_walk(trees, x) for x in Xc[:host_points]]
        t1 = time.perf_counter()
        for mu, var in moments:
            _lib.acq_from_moments(ctx, "ei", 0.0, eta, np.array([mu]), np.array([max(var, 2.0 ** -52)]))
        t2 = time.perf_counter()
        rec["host_pattern"] = {"points": host_points, "walk_ms_per_point": 1e3 * (t1 - t0) / host_points,
                               "acq_from_moments_ms_per_point": 1e3 * (t2 - t1) / host_points}
        rf.close()
    line = json.dumps(rec)
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
