"""Thompson picks by pathwise posterior samples (robo_paths_create, robo_paths_eval_cand) against the EI sweep of the same GP
over the same candidates, at N = 4096, D = 16, 65 536 device-resident candidates, F = 256, 1024, 4096 features and
S = 1, 8, 64 paths, values not copied back.

A   robo_acq_eval_cand, EI, argmax only: as shipped (the acquisition screen on) and with acq_screen = 0 (the full sweep).
B1  robo_paths_create on its own (uploads, Phi_X w, the S-column solve, one synchronisation).
B2  robo_paths_eval_cand with the values not requested; the path kernel from the context's phase events (30 -> 31).
HIP events on the context's stream; medians (min - max) of --reps repetitions after two warm-up rounds, A and B alternating;
one JSON record (stdout, and --out PATH).  The path kernel's rates: its matrix-pipe flops 2 m (N_pad + F_pad) S_pad against
the measured fp64 MFMA peak of the device (diagnostics library), and the (candidate, operand row) pairs per second its
vector pipe forms -- stage 1 and the middle cost the same per pair whatever S is.

    python tools/paths_ab.py [--reps 5] [--out paths_ab.json]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robo_amd import _lib  # noqa: E402
from robo_amd.util.spectral import draw_features  # noqa: E402

N, D, M = 4096, 16, 65536
FS = (256, 1024, 4096)
SS = (1, 8, 64)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": len(ms)}


def timed(ctx, call):
    ctx.record(0)
    out = call()
    ctx.record(1)
    ctx.synchronize()
    return out, ctx.elapsed_ms(0, 1)


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    ctx = _lib.default_context()
    rs = np.random.RandomState(0)
    X = rs.rand(N, D)
    y = np.sinc(X * 10 - 5).sum(axis=1)
    g = _lib.DeviceGP(ctx, "matern52", N, D)
    g.set_data(X, y)
    g.fit(np.concatenate([[0.0], np.full(D, np.log(0.25 * D)), [np.log(1e-3)]]), float(y.mean()))
    cand = _lib.Candidates(ctx, m=M, dim=D, seed=1)
    eta = float(y.min())
    peak = float(ctx.microbench_mfma_f64())
    rec = {"device": ctx.name, "N": N, "D": D, "M": M, "kind": "matern52", "mfma_f64_peak_tflops": peak,
           "note": "one run on one machine", "cases": []}
    ei = {"screen": [], "full": []}
    n_pad = (N + 1 + 127) // 128 * 128
    for F in FS:
        omega, phase = draw_features("matern52", D, F, rs)
        for S in SS:
            w, eps = rs.standard_normal((S, F)), rs.standard_normal((S, N))
            c_ms, e_ms, k_ms = [], [], []
            for r in range(reps + 2):
                for key, knob in (("screen", None), ("full", 0)):
                    ctx.set_tuning("acq_screen", knob)
                    _, t = timed(ctx, lambda: g.acq("ei", 0.0, eta, cand, want_values=False))
                    if r >= 2:
                        ei[key].append(t)
                ctx.set_tuning("acq_screen", None)
                p, tc = timed(ctx, lambda: g.sample_paths(omega, phase, w, eps))
                res, te = timed(ctx, lambda: p.evaluate(cand, want_values=False))
                tk = ctx.elapsed_ms(30, 31)
                p.close()
                if r >= 2:
                    c_ms.append(tc)
                    e_ms.append(te)
                    k_ms.append(tk)
            k = float(np.median(k_ms)) * 1e-3
            f_pad, s_pad = (F + 63) // 64 * 64, (S + 15) // 16 * 16
            rec["cases"].append({"F": F, "S": S, "create": stats(c_ms), "eval": stats(e_ms), "path_kernel": stats(k_ms),
                                 "flags": res.flags, "min0": float(res.min[0]),
                                 "mfma_tflops": 2.0 * M * (n_pad + f_pad) * s_pad / k * 1e-12,
                                 "mfma_fraction_of_peak": 2.0 * M * (n_pad + f_pad) * s_pad / k * 1e-12 / peak,
                                 "gpairs_per_s": M * (n_pad + f_pad) / k * 1e-9})
    rec["ei_screen"], rec["ei_full"] = stats(ei["screen"]), stats(ei["full"])
    for c in rec["cases"]:
        c["eval_over_ei_full"] = c["eval"]["median_ms"] / rec["ei_full"]["median_ms"]
        c["eval_over_ei_screen"] = c["eval"]["median_ms"] / rec["ei_screen"]["median_ms"]
    cand.close()
    g.close()
    line = json.dumps(rec)
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
