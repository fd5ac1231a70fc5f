"""Bayesian linear regression on basis features (robo_blr_*) on the device: what its two hot kernels cost.

A  robo_blr_set_data at N = 2^16 and 2^20 with F = 50 and 128: random Fourier features in D = 8 (kind 3: Phi is never formed)
   and the same Phi passed as rows (kind 0), so that what the feature loader adds -- the x . omega product and the omega
   panel it re-reads from L2 for every 16-row tile -- shows as the difference.  The whole call (upload included) from events
   0 -> 1; the statistics and sum kernels from the phase events 30 -> 31, the eigensolver from 31 -> 29.  The statistics
   kernel's share of the fp64 matrix peak counts 2 N FP^2 flops (FP = F padded to 64 / 128: what the instruction does) against
   --peak-tflops (default 78.6, the MI355X's fp64 matrix figure).
B  robo_blr_acq_eval_cand, EI, 65 536 candidates, S = 20 hyper-parameter samples, F = 128 random Fourier features, values not
   copied back: the call from events 0 -> 1, the sweep kernel from 30 -> 31; against one unscreened EI sweep of an exact GP at
   N = 4096, D = 8 over the same number of device-resident candidates (acq_screen = 0).
HIP events on the context's stream; medians (min - max) of --reps repetitions after two warm-ups; one JSON record (stdout,
and --out PATH).

    python tools/blr_ab.py [--reps 7] [--peak-tflops 78.6] [--out blr_ab.json]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robo_amd import _lib  # noqa: E402

D, M, S, N_GP = 8, 65536, 20, 4096


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": len(ms)}


def timed(ctx, reps, call, pairs):
    """call() reps + 2 times between events 0 and 1 -> {name: stats} for the event pairs {name: (begin, end)}"""
    ms = {name: [] for name in pairs}
    for r in range(reps + 2):
        ctx.record(0)
        call()
        ctx.record(1)
        ctx.synchronize()
        if r >= 2:
            for name, (a, b) in pairs.items():
                ms[name].append(ctx.elapsed_ms(a, b))
    return {name: stats(v) for name, v in ms.items()}


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 7
    peak = float(args[args.index("--peak-tflops") + 1]) if "--peak-tflops" in args else 78.6
    ctx = _lib.default_context()
    ctx.set_phase_events(True)
    ctx.set_tuning("acq_screen", 0)
    rs = np.random.RandomState(0)
    rec = {"device": ctx.name, "D": D, "note": "one run on one machine", "peak_tflops": peak, "set_data": {}}
    pairs = {"call": (0, 1), "stats_kernels": (30, 31), "eig_kernel": (31, 29)}
    for N in (1 << 16, 1 << 20):
        X = rs.rand(N, D)
        y = np.sin(3 * X[:, 0]) + X[:, 1] ** 2 + 0.1 * rs.randn(N)
        for F in (50, 128):
            feat = dict(omega=rs.randn(D, F) * 2.0, phase=rs.rand(F) * 2 * np.pi, scale=float(np.sqrt(2.0 / F)))
            Phi = feat["scale"] * np.cos(X @ feat["omega"] + feat["phase"])
            FP = 64 if F <= 64 else 128
            for kind, rows in (("rff", X), ("given", Phi)):
                h = _lib.DeviceBLR(ctx, kind, D, F, **(feat if kind == "rff" else {}))
                t = timed(ctx, reps, lambda: h.set_data(rows, y), pairs)
                t["stats_share_of_fp64_matrix_peak"] = 2.0 * N * FP * FP / (t["stats_kernels"]["median_ms"] * 1e-3) / (peak * 1e12)
                rec["set_data"]["N%d_F%d_%s" % (N, F, kind)] = t
                h.close()
    N, F = 1 << 16, 128
    X = rs.rand(N, D)
    y = np.sin(3 * X[:, 0]) + X[:, 1] ** 2 + 0.1 * rs.randn(N)
    h = _lib.DeviceBLR(ctx, "rff", D, F, omega=rs.randn(D, F) * 2.0, phase=rs.rand(F) * 2 * np.pi, scale=float(np.sqrt(2.0 / F)))
    h.set_data(X, y)
    h.set_hypers(np.exp(rs.uniform(-2, 6, (S, 2))))
    Xc = rs.rand(M, D)
    rec["sweep"] = timed(ctx, reps, lambda: h.acq("ei", 0.0, float(y.min()), Xc, want_values=False),
                         {"call": (0, 1), "sweep_kernel": (30, 31)})
    h.close()
    g = _lib.DeviceGP(ctx, "matern52", N_GP, D)
    g.set_data(X[:N_GP], y[:N_GP])
    g.fit(np.concatenate([[0.0], np.full(D, np.log(0.25 * D)), [np.log(1e-3)]]), float(y[:N_GP].mean()))
    cand = _lib.Candidates(ctx, m=M, dim=D, seed=1)
    rec["gp_ei_sweep_N4096"] = timed(ctx, reps, lambda: g.acq("ei", 0.0, float(y.min()), cand, want_values=False),
                                     {"call": (0, 1)})
    rec["blr_call_over_gp_call"] = rec["sweep"]["call"]["median_ms"] / rec["gp_ei_sweep_N4096"]["call"]["median_ms"]
    rec["blr_kernel_over_gp_call"] = rec["sweep"]["sweep_kernel"]["median_ms"] / rec["gp_ei_sweep_N4096"]["call"]["median_ms"]
    cand.close()
    g.close()
    ctx.set_tuning("acq_screen", None)
    ctx.set_phase_events(False)
    line = json.dumps(rec)
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
