"""DNGO on the device, measured (NOTES.md): one full-batch Adam step of a 16 -> 3 x 50 -> 1 network at n = 2^10, 2^14, 2^18
(event slots 30 -> 31 around the steps' kernels, the median of `--repeats` calls of `--steps` steps; 28 -> 29 the gradient
kernel's share of it), its fraction of the fp64
matrix peak from 2 n (dim H + (L - 1) H^2) 3 flops per step, the one-launch form against the per-step launches at n = 1024,
and the "mlp" feature kind's robo_blr_set_data and 65 536-candidate sweep against "rff" at the same padded feature count.

    python tools/dngo_ab.py [--repeats 7] [--steps 20] [--out profiles/dngo_ab.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from robo_amd import _lib  # noqa: E402
from robo_amd.models.dngo import glorot_params  # noqa: E402

PEAK_TFLOPS = 78.6     # fp64 matrix peak of the MI355X, the figure README's roofline uses
DIM, H, L, M = 16, 50, 3, 1 << 16


def median_ms(ctx, call, repeats):
    times = []
    for _ in range(repeats + 1):
        call()
        times.append(ctx.elapsed_ms(30, 31))
    return float(np.median(times[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _lib.default_context()
    ctx.set_phase_events(True)
    rs = np.random.RandomState(0)
    p = glorot_params(rs, DIM, L, H)
    mlp = _lib.DeviceMLP(ctx, DIM, L, H)
    res = {"device": ctx.name, "steps_per_call": args.steps, "step": {}}

    def train(X, y):
        mlp.set_params(p)
        mlp.train(X, y, args.steps, 0.01, 1e-4)

    for n in (1 << 10, 1 << 14, 1 << 18):
        X = rs.rand(n, DIM)
        y = np.sin(X.sum(axis=1))
        ctx.set_tuning("mlp_fused", 0)
        ms = median_ms(ctx, lambda: train(X, y), args.repeats) / (args.steps + 1)      # (steps + 1 gradient evaluations)
        flops = 2.0 * n * (DIM * H + (L - 1) * H * H) * 3
        res["step"][str(n)] = {"ms_per_step": ms, "tflops": flops / ms / 1e9, "fraction_of_peak": flops / ms / 1e9 / PEAK_TFLOPS,
                               "gradient_kernel_ms": ctx.elapsed_ms(28, 29)}    # the last call's first gradient launch alone
        if n == 1 << 10:
            ctx.set_tuning("mlp_fused", 1)
            res["one_launch_ms_per_step"] = median_ms(ctx, lambda: train(X, y), args.repeats) / (args.steps + 1)
            res["per_step_ms_per_step"] = ms
        ctx.set_tuning("mlp_fused", None)
    train(X[:4096], y[:4096])
    Xc = rs.rand(M, DIM)
    for kind, kw in (("mlp", dict(mlp=mlp)), ("rff", dict(omega=rs.randn(DIM, H + 1), phase=rs.rand(H + 1), scale=0.2))):
        h = _lib.DeviceBLR(ctx, kind, DIM, H + 1, **kw)
        res[kind + "_set_data_ms"] = median_ms(ctx, lambda: h.set_data(X, y), args.repeats)
        h.set_hypers(np.array([[1.0, 100.0]] * 20))
        res[kind + "_sweep_ms"] = median_ms(ctx, lambda: h.predict(Xc), args.repeats)
        h.close()
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
