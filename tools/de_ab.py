"""Differential evolution on the device (robo_acq_de_cand) against the two host forms of maximizers.DifferentialEvolution,
at N = 4096, D = 16, EI, popsize 240, 20 generations, R = 1 / 8 / 64 populations.

A  one robo_acq_de_cand call (sweep over the R * 240 start members + 20 generations + read-back; Philox draws): HIP events on
   the context's stream and the wall clock around the call, which ends in its one synchronisation.
B  the host maximiser in the reference's form: SciPy drives one 1 x D robo_acq_eval per function value (immediate updating,
   L-BFGS-B polish).  Wall clock; every call synchronises.
C  the host maximiser with batched=True: one robo_acq_eval and one SciPy round trip per generation.  Wall clock.
A and C alternate in one loop, every round with fresh start members (A) and a fresh NumPy seed (C); B, most of a second per
run, is repeated --loop-reps times.  Next to the times: the EI each found and the function values it took (A: R * 240 * 21;
B, C: counted).  B and C end in SciPy's L-BFGS-B polish and A has none, so C's search is also run with polish=False (values
only): that is the like-for-like figure for A's values.  One JSON record (stdout, and --out PATH).  The share of A spent in
de_step_kernel: run `rocprofv3 --kernel-trace --stats -- python tools/de_ab.py --reps 3 --only-a --r 8` on its own.

    python tools/de_ab.py [--reps 10] [--loop-reps 3] [--only-a] [--r 8] [--out de_ab.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scipy import optimize  # noqa: E402

from robo_amd import _lib  # noqa: E402
from robo_amd.maximizers import DifferentialEvolution  # noqa: E402

N, D, NP, T = 4096, 16, 240, 20


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": len(ms)}


def main():
    args = sys.argv[1:]

    def opt(name, default):
        return int(args[args.index(name) + 1]) if name in args else default
    reps, loop_reps = opt("--reps", 10), opt("--loop-reps", 3)
    ctx = _lib.default_context()
    rs = np.random.RandomState(0)
    X = rs.rand(N, D)
    y = np.sinc(X * 10 - 5).sum(axis=1)
    theta = np.concatenate([[0.0], np.full(D, np.log(0.25 * D)), [np.log(1e-3)]])
    g = _lib.DeviceGP(ctx, "matern52", N, D)
    g.set_data(X, y)
    g.fit(theta, float(y.mean()))
    eta = float(y.min())
    count = [0]

    def ei(P):                                   # what an EI object hands a host maximiser: values of the rows of P
        count[0] += len(P)
        return g.acq("ei", 0.0, eta, np.ascontiguousarray(P))[0]

    def host(batched, seed):
        np.random.seed(seed)                     # SciPy draws from the global NumPy stream
        count[0] = 0
        t0 = time.perf_counter()
        x = DifferentialEvolution(ei, np.zeros(D), np.ones(D), n_iters=T, batched=batched).maximize()
        ms = 1e3 * (time.perf_counter() - t0)
        return ms, float(ei(x[None, :])[0]), count[0] - 1
    rec = {"device": ctx.name, "N": N, "D": D, "popsize": NP, "generations": T, "acq": "ei", "note": "one run on one machine"}
    for R in ([opt("--r", 0)] if "--r" in args else [1, 8, 64]):
        ev, wall, a_val, c_ms, c_val = [], [], [], [], []
        for rep in range(reps + 2):              # two warm-up rounds; A and C alternate
            cand = _lib.Candidates(ctx, m=R * NP, dim=D, seed=1 + rep)
            sweep = float(g.acq("ei", 0.0, eta, cand, want_values=False)[1])
            ctx.record(0)
            t0 = time.perf_counter()
            r = g.de("ei", 0.0, eta, cand, R, NP, T, seed=3 + rep)
            t1 = time.perf_counter()
            ctx.record(1)
            ctx.synchronize()
            cand.close()
            if "--only-a" not in args:
                ms, val, nfev = host(True, rep)
            if rep >= 2:
                ev.append(ctx.elapsed_ms(0, 1))
                wall.append(1e3 * (t1 - t0))
                a_val.append(r.value)
                if "--only-a" not in args:
                    c_ms.append(ms)
                    c_val.append(val)
        one = {"A_events": stats(ev), "A_wall": stats(wall), "A_values": a_val, "A_evaluations": R * NP * (T + 1),
               "A_generations_min_max": [int(min(r.generations)), int(max(r.generations))], "A_flags": r.flags,
               "last_sweep_value": sweep}
        if "--only-a" not in args:
            one.update(C_batched=stats(c_ms), C_values=c_val, C_evaluations=nfev, A_over_C=float(np.median(wall) / np.median(c_ms)))
        rec["R%d" % R] = one
    if "--only-a" not in args:
        plain = []
        for seed in range(reps):                 # C's search without the polish: values only
            np.random.seed(2 + seed)
            found = optimize.differential_evolution(lambda pop: -ei(np.ascontiguousarray(pop.T)), [(0.0, 1.0)] * D, maxiter=T,
                                                    vectorized=True, updating="deferred", polish=False)
            plain.append(float(-found["fun"]))
        rec["C_values_without_polish"] = plain
        runs = [host(False, s) for s in range(loop_reps + 1)][1:]
        rec["B_reference_form"] = dict(stats([a[0] for a in runs]), values=[a[1] for a in runs], evaluations=[a[2] for a in runs])
    g.close()
    line = json.dumps(rec)
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
