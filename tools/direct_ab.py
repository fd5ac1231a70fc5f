"""DIRECT on the device against a host loop of the same rule (NOTES.md "DIRECT on the device").

    python tools/direct_ab.py [--n 4096] [--reps 5] [--out profiles/direct_ab_mi355x.json]

Per D in (16, 2), N = 4096, LogEI: A = one robo_acq_direct call at the reference's budget (400 values, 200 iterations) and at
1e4 values; B = tests/direct_oracle.py's rule on the host around ONE robo_acq_eval_cand call of `batch` rows per iteration
(the host form pays a launch chain, a synchronisation and Python per iteration, not per point as the reference does).  Wall
clock around calls that end in a synchronisation, one warm-up, medians of --reps.  Also: deferred iterations at the default
batch, the value reached beside maximizer "cmaes" and "device_gradient" on the same model, and the posterior's share of A,
estimated as T eager posterior batches of the same rows over A's time (no events inside the call).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import direct_oracle as DO  # noqa: E402
from robo_amd import _lib  # noqa: E402


def median_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def host_loop(ctx, g, eta, D, B, max_evals, max_iters):
    o = DO.Direct(D, B, 1e-4, max_evals, 0)
    rows = np.full((B, D), 0.5)
    cand = _lib.Candidates(ctx, rows)
    o.start(g.acq("log_ei", 0.0, eta, cand)[0][0])
    for _ in range(max_iters):
        sel = o.select()
        if sel["stop"]:
            break
        rows[:] = sel["x"][0]
        rows[:len(sel["x"])] = sel["x"]
        cand.set_points(rows)
        o.divide(sel, g.acq("log_ei", 0.0, eta, cand)[0][:len(sel["x"])])
    cand.close()
    best, fmin = o.best()
    return o.c[best], -fmin, len(o.f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx, res = _lib.default_context(0), {"n": a.n, "device": None}
    res["device"] = ctx.name
    for D in (16, 2):
        rs = np.random.RandomState(D)
        X = rs.rand(a.n, D)
        y = np.sin(3 * X.sum(axis=1) / np.sqrt(D / 3.0)) + 0.1 * rs.randn(a.n)
        g = _lib.DeviceGP(ctx, "matern52", a.n, D)
        g.set_data(X, y)
        g.fit(np.concatenate([[0.0], np.log(np.full(D, 0.25 * np.sqrt(D))), [np.log(1e-2)]]), float(y.mean()))
        eta, B, row = float(y.min()), _lib.direct_default_batch(D), {}
        for name, E, T in (("ref_budget", 400, 200), ("1e4", 10000, 200)):
            r = g.direct("log_ei", 0.0, eta, E, T, diagnostics=True)
            deferred = int(np.sum((r.trace["flags"].astype(np.int64) & DO.DEFERRED != 0) & (r.trace["ran"] == 1)))
            first = int(np.argmax(r.trace["flags"].astype(np.int64) & DO.DEFERRED != 0)) if deferred else -1
            ms = median_ms(lambda: g.direct("log_ei", 0.0, eta, E, T), a.reps)
            cand = _lib.Candidates(ctx, r.trace["x"][1])
            post = median_ms(lambda: g.acq("log_ei", 0.0, eta, cand), a.reps)
            cand.close()
            enq = len(r.trace["ran"])
            row[name] = dict(ms=ms, value=r.value, evals=r.evals, iters=r.iters, enqueued=enq - 1, flags=r.flags,
                             rows_with_deferral_flag=deferred, first_deferral=first, eager_batch_ms=post,
                             posterior_share_estimate=min(1.0, post * enq / ms))
        host_loop(ctx, g, eta, D, B, 400, 200)
        t0 = time.perf_counter()
        hx, hv, he = host_loop(ctx, g, eta, D, B, 400, 200)
        host_ms = (time.perf_counter() - t0) * 1e3
        r = g.direct("log_ei", 0.0, eta, 400, 200)
        row["host_loop"] = dict(ms=host_ms, value=hv, evals=he, same_point=bool(np.array_equal(hx, r.x)),
                                same_value=bool(hv == r.value))
        cand = _lib.Candidates(ctx, m=65536, seed=1, n_uniform=65536, loc=np.full(D, 0.5), scale=np.full(D, 0.1))
        row["cmaes_value"] = g.cmaes("log_ei", 0.0, eta, cand, 4, None, 100).value
        row["device_gradient_value"] = g.refine("log_ei", 0.0, eta, cand, 256, 50, 0.05).value
        row["sweep_value"] = g.acq("log_ei", 0.0, eta, cand, want_values=False)[1]
        cand.close()
        g.close()
        res["D%d" % D] = row
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
