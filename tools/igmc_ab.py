"""Monte-Carlo entropy search: the device (robo_igmc_eval_cand: cross-covariances, variances and the MC gains of a whole
candidate batch in one call) against the NumPy oracle of tests/igmc_oracle.py, at the reference's defaults Nb = 50,
Np = 50, Nf = 500, for M = 500 and 8192 candidates.  Device: synchronised wall clock after warm-up.  Host: the oracle's
per-candidate loop on --host-max candidates (all of them for M <= host-max), extrapolated linearly to M and labelled so.
Agreement: counts and gains on 64 of those candidates, near-tie draws (tests/igmc_oracle.py) excluded.  Writes one JSON
record (stdout, and --out PATH).  Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/igmc_ab.py`.

    python tools/igmc_ab.py [--reps 7] [--host-max 500] [--out igmc_ab.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import igmc_oracle as MO  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402
from robo_amd import _lib  # noqa: E402
from robo_amd.acquisition_functions.information_gain import outcome_quantiles  # noqa: E402


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()                                  # the entry point returns after the stream has synchronised
        out.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * float(np.median(out)), "min_ms": 1e3 * min(out), "max_ms": 1e3 * max(out), "reps": reps}


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 7
    host_max = int(args[args.index("--host-max") + 1]) if "--host-max" in args else 500
    ctx = _lib.default_context()
    Nb, Np, Nf, N, D = 50, 50, 500, 200, 3
    rs = np.random.RandomState(0)
    X = rs.rand(N, D)
    y = np.sin(3 * X.sum(axis=1)) + 0.1 * rs.randn(N)
    theta = np.concatenate([[0.0], np.log([0.3, 0.5, 0.8]), [np.log(1e-2)]])
    ogp = O.OracleGP("matern52", theta, normalize_input=False)
    ogp.train(X, y)
    g = _lib.DeviceGP(ctx, "matern52", N, D)
    g.set_data(X, y)
    g.fit(theta, ogp.mean)
    sn2 = float(np.exp(theta[-1]))
    zb = rs.rand(Nb, D)
    Mb, Vb = ogp.predict(zb, full_cov=True)
    Mb, Vb = np.asarray(Mb).ravel(), np.asarray(Vb)
    z = rs.randn(Nf, Nb)
    W = outcome_quantiles(Np).ravel()
    lmb = rs.randn(Nb)
    t0 = time.perf_counter()
    p0, _ = MO.pmin_mc(Mb, Vb, z)
    host_pmin_ms = 1e3 * (time.perf_counter() - t0)
    logP = np.log(p0)
    mc = _lib.MCState(z, Mb, Vb, logP, lmb, W)
    rec = {"device": ctx.name, "Nb": Nb, "Np": Np, "Nf": Nf, "N": N, "D": D, "note": "one run on one machine",
           "pmin": {"device": timed(lambda: _lib.pmin_mc(ctx, Mb[None], Vb[None], z), reps), "host_ms": host_pmin_ms,
                    "bit_equal": bool(np.array_equal(_lib.pmin_mc(ctx, Mb[None], Vb[None], z)[0][0], p0))}}
    rep = _lib.Candidates(ctx, zb)
    for M in (500, 8192):
        Xc = rs.rand(M, D)
        cand = _lib.Candidates(ctx, Xc)
        dev = timed(lambda: _lib.igmc_eval(g, cand, rep, mc, sn2), reps)
        vals, mx, am, flags = _lib.igmc_eval(g, cand, rep, mc, sn2)
        S = _lib.cross_cov(g, cand, rep)
        _, var = g.predict(cand)
        cand.close()
        k = min(M, host_max)
        sub = np.sort(np.random.RandomState(M).choice(M, k, replace=False))
        t0 = time.perf_counter()
        MO.gains(S[sub], var[sub], sn2, Mb, Vb, logP, lmb, W, z, ties=False)
        host_s = time.perf_counter() - t0
        sub = sub[:64]                       # agreement, near ties detected (a sort per draw: not part of the timing)
        o = MO.gains(S[sub], var[sub], sn2, Mb, Vb, logP, lmb, W, z)
        tie_c = o["tie"].any(axis=(1, 2))
        clean = ~tie_c
        rec["M%d" % M] = {
            "device": dev,
            "host_ms": 1e3 * host_s * M / k,
            "host_measured_candidates": int(k),
            "host_extrapolated": bool(k < M),
            "speedup": 1e3 * host_s * M / k / dev["median_ms"],
            "flags": int(flags),
            "near_tie_draws": int(o["tie"].sum()),
            "candidates_with_near_ties": int(tie_c.sum()),
            "counts_equal_where_no_tie": bool(np.array_equal(
                _lib.igmc_from_moments(ctx, S[sub][clean], var[sub][clean], mc, sn2, with_counts=True)[1],
                o["counts"][clean])),
            "max_rel_gain_diff_where_no_tie": float(np.max(np.abs(vals[sub][clean] - o["gain"][clean]) /
                                                           np.maximum(np.abs(o["gain"][clean]), 1e-300)))
            if clean.any() else None,
        }
    rep.close()
    g.close()
    line = json.dumps(rec)
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
