"""BOHAMIANN on the device, measured (NOTES.md): SGHMC steps per second of 1, 8 and 64 chains at n = 200, D = 16 and the default
net (event slots 30 -> 31 around the chain launches, the median of `--repeats` calls of `--steps` steps past the burn-in and
inside it), and the ensemble sweep of S = 100 networks over 65 536 candidates (30 -> 31 around the sweep kernel, and the whole
call by the wall clock) against the only route there was before it: S calls of robo_mlp_forward and a NumPy fold (wall clock).
The sweep's fraction of the fp64 matrix peak counts 2 m S (dim H + (L - 1) H^2 + H) flops.

    python tools/bohamiann_ab.py [--repeats 7] [--steps 2000] [--out profiles/bohamiann_ab.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from robo_amd import _lib  # noqa: E402
from robo_amd.models.bohamiann import kaiming_params  # noqa: E402

PEAK_TFLOPS = 78.6     # fp64 matrix peak of the MI355X, the figure README's roofline uses
N, DIM, H, L, M, S = 200, 16, 50, 2, 1 << 16, 100


def median(ctx, call, repeats, events=True):
    times = []
    for _ in range(repeats + 1):
        t0 = time.perf_counter()
        call()
        times.append(ctx.elapsed_ms(30, 31) if events else 1e3 * (time.perf_counter() - t0))
    return float(np.median(times[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _lib.default_context()
    ctx.set_phase_events(True)
    rs = np.random.RandomState(0)
    X = rs.rand(N, DIM)
    y = np.sin(X.sum(axis=1))
    res = {"device": ctx.name, "steps_per_call": args.steps, "chains": {}}
    for C in (1, 8, 64):
        bnn = _lib.DeviceBNN(ctx, DIM, L, H, C)
        bnn.set_state(np.stack([kaiming_params(rs, DIM, L, H) for _ in range(C)]))
        row = {}
        for name, burn in (("burn_in", 1 << 30), ("sampling", 0)):      # (burn-in first: the sampling steps need its V)
            ms = median(ctx, lambda: bnn.run(X, y, args.steps, burn, 1 << 30, 20, 1e-2, 0.05, seed=1), args.repeats)
            row[name + "_steps_per_s"] = 1e3 * args.steps / ms
            row[name + "_chain_steps_per_s"] = 1e3 * args.steps * C / ms
        res["chains"][str(C)] = row
        bnn.close()
    samples = np.stack([kaiming_params(rs, DIM, L, H) for _ in range(S)])
    Xc = rs.rand(M, DIM)
    bnn = _lib.DeviceBNN(ctx, DIM, L, H)
    bnn.set_samples(samples)
    mlp = _lib.DeviceMLP(ctx, DIM, L, H)

    def parent_route():
        f = np.empty((S, M))
        for s in range(S):
            mlp.set_params(samples[s, :-1])
            f[s] = mlp.forward(Xc)[1]
        return f.mean(axis=0), f.var(axis=0)

    res["sweep_kernel_ms"] = median(ctx, lambda: bnn.predict(Xc), args.repeats)
    res["sweep_call_ms"] = median(ctx, lambda: bnn.predict(Xc), args.repeats, events=False)
    res["parent_route_ms"] = median(ctx, parent_route, max(args.repeats // 2, 1), events=False)
    res["ratio_call"] = res["parent_route_ms"] / res["sweep_call_ms"]
    flops = 2.0 * M * S * (DIM * H + (L - 1) * H * H + H)
    res["sweep_tflops"] = flops / res["sweep_kernel_ms"] / 1e9
    res["sweep_fraction_of_peak"] = res["sweep_tflops"] / PEAK_TFLOPS
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
