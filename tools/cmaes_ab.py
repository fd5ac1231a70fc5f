"""CMA-ES on the device (robo_acq_cmaes_cand) against what the library offered before it, at N = 4096, D = 16, LogEI,
65 536 device-resident candidates, R = 1 / 16 / 64 instances of lambda = 12 / 32 samples and T = 100 generations.

A  the new call: T = 0 (sweep + selection) and T = 100, alternating; the difference of each pair is the generations alone
   (median, min, max over the pairs), divided by T the time per generation.  HIP events on the context's stream.
B  the same generations as a host loop: one robo_acq_eval of the R lambda points per generation and the update of every
   instance in NumPy (what a user could write before): wall clock, every call synchronises.  Device and host loop are
   also run once from the same caller-supplied draws: their values side by side check the algorithm, not the clock.
Also: the final LogEI next to robo_acq_refine_cand's at the same number of acquisition evaluations (K = R lambda starts,
T steps: K (T + 1) values and gradients).  One JSON record (stdout, and --out PATH).  Kernel shares: run
`rocprofv3 --kernel-trace --stats -- python tools/cmaes_ab.py --reps 3 --only-a --r 16 --lam 12` on its own.

    python tools/cmaes_ab.py [--reps 10] [--loop-reps 5] [--only-a] [--r 16] [--lam 12] [--out cmaes_ab.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cmaes_oracle as CO  # noqa: E402
from robo_amd import _lib  # noqa: E402

N, D, M, T, SIGMA0 = 4096, 16, 65536, 100, 0.25


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": len(ms)}


def host_loop(g, eta, starts, f0, lam, zs):
    """the algorithm of robo_acq_cmaes_cand from the means `starts` and the draws zs (T, R, lam, D) with robo_acq_eval and
    NumPy on the host"""
    R, n = starts.shape
    K = dict(CO.constants(n, lam))
    K.update(me=K["mueff"], every=CO.default_eig_every(n, K))
    m, sig, ps, pc = starts.copy(), np.full(R, SIGMA0), np.zeros((R, n)), np.zeros((R, n))
    C, A, Ai, best = np.tile(np.eye(n), (R, 1, 1)), np.tile(np.eye(n), (R, 1, 1)), np.tile(np.eye(n), (R, 1, 1)), f0.copy()
    for t, z in enumerate(zs):
        x = np.clip(m[:, None, :] + sig[:, None, None] * np.einsum("rde,rle->rld", A, z), 0.0, 1.0)
        y = (x - m[:, None, :]) / sig[:, None, None]
        f = g.acq("log_ei", 0.0, eta, x.reshape(-1, n))[0].reshape(R, lam)
        ys = np.take_along_axis(y, np.argsort(-f, axis=1, kind="stable")[:, :K["mu"], None], axis=1)
        yw = np.einsum("k,rkd->rd", K["w"], ys)
        m = np.clip(m + sig[:, None] * yw, 0.0, 1.0)
        ps = (1 - K["cs"]) * ps + np.sqrt(K["cs"] * (2 - K["cs"]) * K["me"]) * np.einsum("rde,re->rd", Ai, yw)
        pn = np.sqrt((ps ** 2).sum(axis=1))
        hs = (pn / np.sqrt(1 - (1 - K["cs"]) ** (2 * (t + 1))) < (1.4 + 2 / (n + 1)) * K["chin"]).astype(float)
        pc = (1 - K["cc"]) * pc + (hs * np.sqrt(K["cc"] * (2 - K["cc"]) * K["me"]))[:, None] * yw
        keep = 1 - K["c1"] - K["cmu"] + K["c1"] * (1 - hs) * K["cc"] * (2 - K["cc"])
        C = keep[:, None, None] * C + K["c1"] * pc[:, :, None] * pc[:, None, :] + \
            K["cmu"] * np.einsum("k,rkd,rke->rde", K["w"], ys, ys)
        sig = sig * np.exp(K["cs"] / K["ds"] * (pn / K["chin"] - 1))
        if (t + 1) % K["every"] == 0:
            lam_, B = np.linalg.eigh(C)
            A = np.einsum("rdk,rk,rek->rde", B, np.sqrt(lam_), B)
            Ai = np.einsum("rdk,rk,rek->rde", B, 1 / np.sqrt(lam_), B)
        best = np.maximum(best, f.max(axis=1))
    return best.max()


def main():
    args = sys.argv[1:]

    def opt(name, default):
        return int(args[args.index(name) + 1]) if name in args else default
    reps, loop_reps = opt("--reps", 10), opt("--loop-reps", 5)
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
    vals, sweep_value = g.acq("log_ei", 0.0, eta, cand)[:2]
    rec = {"device": ctx.name, "N": N, "D": D, "M": M, "T": T, "acq": "log_ei", "sweep_value": float(sweep_value),
           "note": "one run on one machine"}
    for R in ([opt("--r", 0)] if "--r" in args else [1, 16, 64]):
        for lam in ([opt("--lam", 0)] if "--lam" in args else [12, 32]):
            legs = {0: [], T: []}
            for rep in range(reps + 2):          # the two legs alternate: every repetition yields its own difference
                for gens in (0, T):
                    ctx.record(0)
                    r = g.cmaes("log_ei", 0.0, eta, cand, R, lam, gens, SIGMA0, seed=3)
                    ctx.record(1)
                    ctx.synchronize()
                    if rep >= 2:
                        legs[gens].append(ctx.elapsed_ms(0, 1))
            only = stats([b - a for a, b in zip(legs[0], legs[T])])
            k = min(R * lam, 1024)
            ref = g.refine("log_ei", 0.0, eta, cand, k, max(0, R * lam * T // k - 1), 0.05)
            one = {"A_sweep_select": stats(legs[0]), "A_all": stats(legs[T]), "A_generations_only": only,
                   "A_ms_per_generation": only["median_ms"] / T, "value": r.value, "flags": r.flags,
                   "refine_value_same_evaluations": ref.value, "refine_starts": k}
            if "--only-a" not in args:
                # the same draws for both: the device's value next to the host loop's is then a check of the algorithm
                order = np.argsort(-vals, kind="stable")[:R]
                zs = np.random.RandomState(3).standard_normal((T, R, lam, D))
                one["value_same_z"] = g.cmaes("log_ei", 0.0, eta, cand, R, lam, T, SIGMA0, z=zs).value
                t = []
                for _ in range(loop_reps + 1):
                    t0 = time.perf_counter()
                    fb = host_loop(g, eta, cand.points()[order], vals[order], lam, zs)
                    t.append(1e3 * (time.perf_counter() - t0))
                one.update(B_host_loop=stats(t[1:]), B_value_same_z=float(fb),
                           B_over_A=float(np.median(t[1:])) / only["median_ms"])
            rec["R%d_lambda%d" % (R, lam)] = one
    cand.close()
    g.close()
    line = json.dumps(rec)
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
