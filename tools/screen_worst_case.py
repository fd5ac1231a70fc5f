"""The acquisition screen's worst case at the headline shape: eta lowered by 5, so that nothing is pruned, the probe runs,
the call falls back to the plain sweep and the back-off skips the screen for 1, 2, 4, ... calls.  Eight argmax-only EI calls
after a refit, ms per call, and the answer.

    python tools/screen_worst_case.py [--lib path/to/librobo_hip.so] [--n 4096] [--d 16] [--m 65536]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robo_amd import _lib  # noqa: E402
from bench import synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--m", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=8)
    args = ap.parse_args()
    if args.lib:
        _lib.use_library(os.path.abspath(args.lib))
    ctx = _lib.Context(0)
    X, y, theta, Xc = synthetic(args.n, args.d, args.m, 0)
    gp = _lib.DeviceGP(ctx, "matern52", args.n, args.d)
    gp.set_data(X, y)
    cand = _lib.Candidates(ctx, Xc)
    mean_c, eta = float(y.mean()), float(y.min()) - 5.0
    gp.fit(theta, mean_c)
    gp.acq("ei", 0.0, float(y.min()), cand, want_values=False)         # warm-up: buffers, alpha, the sub-handle
    gp.fit(theta, mean_c)                                              # a refit: the back-off starts afresh
    ms, outcomes, res = [], [], None
    for _ in range(args.calls):
        t0 = time.perf_counter()
        res = gp.acq("ei", 0.0, eta, cand, want_values=False)[1:]
        ms.append(round((time.perf_counter() - t0) * 1e3, 3))
        outcomes.append(cand.last_screen()[2])
    print(json.dumps({"lib": args.lib or "default", "ms_per_call": ms, "outcomes": outcomes,
                      "result": [res[0], int(res[1]), int(res[2])]}))
    cand.close()
    gp.close()
    ctx.close()


if __name__ == "__main__":
    main()
