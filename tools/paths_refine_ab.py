"""Refinement of Thompson picks on the paths (robo_paths_refine_cand) against what the sweep alone offers for the same goal, at
N = 4096, D = 16, F = 1024 features, 65 536 device-generated candidates, S = 1, 8, 64 paths, n_starts = 16, 64, 256 per path,
T = 50 steps, step0 = 0.05.

A   the fused call without steps (T = 0: the sweep, the start selection, the winners) and with T = 50, alternating; HIP
    events on the context's stream around each call; the per-pair difference is the refinement.  The descent launch alone
    from the context's event slots 28 -> 29: (path, point) x (training row or feature) pairs per second per evaluation,
    P (T + 1) (N + F) / time, next to the sweep kernel's rate (slots 30 -> 31) measured in the same run.
B   robo_paths_eval_cand sweeps of 2^16 .. 2^20 candidates on the same paths object (values not requested) and the minimum
    each reaches per path: what more candidates buy instead of descents.
Medians (min - max) of --pairs repetitions after two warm-up rounds; one JSON record per (S, n_starts) and one per sweep size
on stdout, and appended to --out PATH.  --lib PATH measures another build of the library (the workgroup-shape comparison of
NOTES.md "Refining a path's minimiser" was made this way).

    python tools/paths_refine_ab.py [--pairs 20] [--out paths_refine_ab.json] [--lib PATH] [--label TEXT]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robo_amd import _lib  # noqa: E402
from robo_amd.util.spectral import draw_features  # noqa: E402

N, D, M, F, T, STEP0 = 4096, 16, 65536, 1024, 50, 0.05
SS = (1, 8, 64)
KS = (16, 64, 256)
SWEEPS = (2 ** 16, 2 ** 17, 2 ** 18, 2 ** 19, 2 ** 20)


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
    opt = lambda k, d: args[args.index(k) + 1] if k in args else d  # noqa: E731
    pairs, out, label = int(opt("--pairs", 20)), opt("--out", None), opt("--label", "as built")
    if "--lib" in args:
        _lib.use_library(opt("--lib", None))
    ctx = _lib.default_context()
    rs = np.random.RandomState(0)
    X = rs.rand(N, D)
    y = np.sinc(X * 10 - 5).sum(axis=1)
    g = _lib.DeviceGP(ctx, "matern52", N, D)
    g.set_data(X, y)
    g.fit(np.concatenate([[0.0], np.full(D, np.log(0.25 * D)), [np.log(1e-3)]]), float(y.mean()))
    omega, phase = draw_features("matern52", D, F, rs)
    cands = {m: _lib.Candidates(ctx, m=m, dim=D, seed=1) for m in SWEEPS}
    cand = cands[M]

    def emit(rec):
        rec.update({"device": ctx.name, "label": label, "N": N, "D": D, "F": F, "kind": "matern52",
                    "note": "one run on one machine"})
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            with open(out, "a") as fh:
                fh.write(line + "\n")

    for S in SS:
        w, eps = rs.standard_normal((S, F)), rs.standard_normal((S, N))
        p = g.sample_paths(omega, phase, w, eps)
        for K in KS:
            t0, t1, kd, ks = [], [], [], []
            for r in range(pairs + 2):
                r0, a = timed(ctx, lambda: p.refine(cand, K, 0, STEP0))
                r1, b = timed(ctx, lambda: p.refine(cand, K, T, STEP0))
                if r >= 2:
                    t0.append(a)
                    t1.append(b)
                    kd.append(ctx.elapsed_ms(28, 29))
                    ks.append(ctx.elapsed_ms(30, 31))
            P = S * K
            sec = float(np.median(kd)) * 1e-3
            emit({"what": "refine", "S": S, "n_starts": K, "T": T, "M": M, "fused_T0": stats(t0), "fused_T": stats(t1),
                  "refinement": stats([b - a for a, b in zip(t0, t1)]), "descent_launch": stats(kd), "sweep_kernel": stats(ks),
                  "descent_gpairs_per_s": P * (T + 1) * (N + F) / sec * 1e-9,
                  "sweep_gpairs_per_s": M * (N + F) / (float(np.median(ks)) * 1e-3) * 1e-9,
                  "refinement_over_sweep_call": float(np.median([b - a for a, b in zip(t0, t1)])) / float(np.median(t0)),
                  "flags": r1.flags, "sweep_best": r0.value.tolist(), "refined_min": r1.value.tolist()})
        for m in SWEEPS:
            ms = []
            for r in range(7):
                res, t = timed(ctx, lambda: p.evaluate(cands[m], want_values=False))
                if r >= 2:
                    ms.append(t)
            emit({"what": "sweep", "S": S, "M": m, "eval": stats(ms), "flags": res.flags, "min": res.min.tolist()})
        p.close()
    for c in cands.values():
        c.close()
    g.close()


if __name__ == "__main__":
    main()
