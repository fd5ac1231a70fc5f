"""Entropy search's update() with the representer chains on the host against on the device, one MI355X.

MarginalizationGPMCMC(InformationGain).update over S = 20 fitted sub-models at N in {100, 200, 1000}, D = 4, Nb = 50,
50 sampler steps, ep="device" in both legs:

A  representers="host": per estimator 100 half-steps, each one robo_acq_eval round trip (the code path of the parent).
B  representers="device": one robo_rep_sample_batch for all S chains, then predict_cov per estimator and one batched EP.

Wall-clock of update() (it ends synchronised: the EP state comes back to the host), split into chain / predict_cov / EP
by timing the calls those parts go through; medians (min - max) of --reps repetitions after a warm-up, A and B
alternating; launches per half-step of B from the solve's block rows.  One JSON record (stdout, and --out PATH).

    python tools/rep_ab.py [--reps 5] [--sizes 100,200,1000] [--out rep_ab.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robo_amd import _lib  # noqa: E402
from robo_amd.acquisition_functions import EI, InformationGain, MarginalizationGPMCMC  # noqa: E402
from robo_amd.kernels import Matern52Kernel  # noqa: E402
from robo_amd.models.gaussian_process import GaussianProcess  # noqa: E402

D, NB, STEPS, S = 4, 50, 50, 20


class Samples(object):
    """stands in for a trained GaussianProcessMCMC: MarginalizationGPMCMC reads ``models``"""

    def __init__(self, models):
        self.models = models


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": len(ms)}


class Clock(object):
    """accumulates the wall-clock spent inside wrapped callables"""

    def __init__(self):
        self.ms = {}

    def wrap(self, owner, name, part):
        real = getattr(owner, name)

        def timed(*a, **kw):
            t0 = time.perf_counter()
            try:
                return real(*a, **kw)
            finally:
                self.ms[part] = self.ms.get(part, 0.0) + 1e3 * (time.perf_counter() - t0)
        setattr(owner, name, timed)
        return lambda: setattr(owner, name, real)


def build(n, representers):
    rs = np.random.RandomState(0)
    lo, hi = np.zeros(D), np.ones(D)
    X = rs.rand(n, D)
    y = np.sinc(X * 10 - 5).sum(axis=1)
    subs = []
    for s in range(S):
        m = GaussianProcess(2 * Matern52Kernel(np.full(D, 0.2 * (1 + 0.05 * s)), ndim=D), noise=1e-3 * (1 + 0.1 * s), lower=lo,
                            upper=hi, rng=np.random.RandomState(3))
        m.train(X, y, do_optimize=False)
        subs.append(m)
    model = Samples(subs)
    base = InformationGain(model, lo, hi, Nb=NB, sampling_acquisition=EI, rng=np.random.RandomState(1), ep="device",
                           representers=representers)
    base.sampler_steps = STEPS
    return model, MarginalizationGPMCMC(base)


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    sizes = [int(x) for x in args[args.index("--sizes") + 1].split(",")] if "--sizes" in args else [100, 200, 1000]
    ctx = _lib.default_context()
    rec = {"device": ctx.name, "D": D, "Nb": NB, "steps": STEPS, "S": S, "note": "one run on one machine", "sizes": {}}
    for n in sizes:
        legs = {name: build(n, name) for name in ("host", "device")}
        clock = Clock()
        undo = [clock.wrap(InformationGain, "sample_representer_points", "chain"),
                clock.wrap(_lib, "rep_sample_batch", "chain"),
                clock.wrap(_lib.DeviceGP, "predict_cov", "predict_cov"),
                clock.wrap(_lib, "ep_joint_min", "ep")]
        total = {name: [] for name in legs}
        parts = {name: {"chain": [], "predict_cov": [], "ep": []} for name in legs}
        warm = 2
        try:
            for rep in range(reps + warm):
                for name, (model, marg) in legs.items():
                    clock.ms = {}
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    marg.update(model)
                    ms = 1e3 * (time.perf_counter() - t0)
                    if rep >= warm:
                        total[name].append(ms)
                        for part in parts[name]:
                            parts[name][part].append(clock.ms.get(part, 0.0))
        finally:
            for u in undo:
                u()
        nbk = (n + 127) // 128
        launches = 2 + S * (nbk + 1)            # propose + accept for all chains; per chain the block rows of the solve + post
        out = {name: {"update": stats(total[name]), **{p: stats(v) for p, v in parts[name].items()}} for name in legs}
        out["host_over_device"] = out["host"]["update"]["median_ms"] / out["device"]["update"]["median_ms"]
        out["chain_host_over_device"] = out["host"]["chain"]["median_ms"] / out["device"]["chain"]["median_ms"]
        out["device_launches_per_half_step"] = launches
        out["device_us_per_half_step"] = 1e3 * out["device"]["chain"]["median_ms"] / (2 * STEPS + 2)
        out["device_us_per_launch"] = out["device_us_per_half_step"] / launches
        rec["sizes"][str(n)] = out
        for model, _ in legs.values():
            for m in model.models:
                m.gp.close()
    line = json.dumps(rec)
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
