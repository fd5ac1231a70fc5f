"""Greedy batch proposals on the device (robo_acq_batch_cand) against the loop a user had to write before it, at
N = 4096, D = 16, EI, 65 536 device-resident candidates, q = 8.

A  robo_acq_batch_cand with q = 8 (kriging believer), and with q = 1 (= one sweep): HIP events on the context's stream.
   (A(q = 8) - A(q = 1)) / 7 is the cost of a pick after the first.
B  the loop: eight times { robo_gp_set_data with the fantasy point appended, robo_gp_fit at the same theta,
   robo_acq_eval_cand }: wall clock (every call synchronises), same picks' worth of work.
C  one sweep, robo_acq_eval_cand.
Medians (min - max) of --reps repetitions after a warm-up; one JSON record (stdout, and --out PATH).  Kernel shares: run
under `rocprofv3 --kernel-trace --stats -- python tools/batch_ab.py --reps 3 --only-a`.

    python tools/batch_ab.py [--reps 5] [--only-a] [--out batch_ab.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robo_amd import _lib  # noqa: E402

N, D, M, Q = 4096, 16, 65536, 8


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


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    ctx = _lib.default_context()
    rs = np.random.RandomState(0)
    X = rs.rand(N, D)
    y = np.sinc(X * 10 - 5).sum(axis=1)
    theta = np.concatenate([[0.0], np.full(D, np.log(0.25 * D)), [np.log(1e-3)]])
    mean = float(y.mean())
    g = _lib.DeviceGP(ctx, "matern52", N + Q, D)
    g.set_data(X, y)
    g.fit(theta, mean)
    eta = float(y.min())
    cand = _lib.Candidates(ctx, m=M, dim=D, seed=1)
    rec = {"device": ctx.name, "N": N, "D": D, "M": M, "q": Q, "acq": "ei", "fantasy": "kriging_believer",
           "note": "one run on one machine"}
    rec["C_one_sweep"] = events(ctx, lambda: g.acq("ei", 0.0, eta, cand, want_values=False), reps)
    legs = {1: [], Q: []}
    for rep in range(reps + 2):                   # the two legs alternate: every repetition yields its own difference
        for q in (1, Q):
            ctx.record(0)
            r = g.select_batch("ei", 0.0, eta, cand, q)
            ctx.record(1)
            ctx.synchronize()
            if rep >= 2:
                legs[q].append(ctx.elapsed_ms(0, 1))
    rec["A_q1"], rec["A_q8"] = stats(legs[1]), stats(legs[Q])
    rec["A_per_later_pick"] = stats([(b - a) / (Q - 1) for a, b in zip(legs[1], legs[Q])])
    rec["A_picks"] = [int(i) for i in r.indices]
    if "--only-a" not in args:
        Xc = cand.points()
        t, picks = [], []
        for rep in range(reps + 1):
            g.set_data(X, y)
            g.fit(theta, mean)
            Xa, ya, e, picks = X, y, eta, []
            t0 = time.perf_counter()
            for j in range(Q):
                if j:
                    g.set_data(Xa, ya)
                    g.fit(theta, mean)
                _, mx, am, _ = g.acq("ei", 0.0, e, cand, want_values=False)
                picks.append(int(am))
                # the kriging believer's target: the posterior mean at the pick (one more small call, as a user would)
                yf = float(g.predict(Xc[am:am + 1])[0][0])
                Xa, ya, e = np.vstack([Xa, Xc[am]]), np.append(ya, yf), min(e, yf)
            t.append(1e3 * (time.perf_counter() - t0))
        rec["B_refit_loop"] = stats(t[1:])
        rec["B_picks"] = picks
        rec["B_over_A"] = rec["B_refit_loop"]["median_ms"] / rec["A_q8"]["median_ms"]
        rec["same_picks"] = picks == rec["A_picks"]
    cand.close()
    g.close()
    line = json.dumps(rec)
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
