"""Acquisition maximisation by CMA-ES on the device.

``CMAES`` has the signature of robo/maximizers/cmaes.py (which drives the ``cma`` package from the host, one 1 x D
acquisition call per function value); everything else sits behind the reference's parameters.  It draws
:class:`DeviceGradientAscent`'s candidates (70 % uniform over the box, 30 % N(incumbent, 0.1) clipped; Philox, seeded from
the maximiser's rng), scores them with one fused acquisition call and starts ``restarts + 1`` independent
(mu/mu_w, lambda)-CMA-ES instances from the best of them.  The instances run SIDE BY SIDE in lock step without leaving
the device (robo_acq_cmaes_cand / robo_acq_cmaes_marginal_cand), ``max(1, n_func_evals // popsize)`` generations each:
global, derivative-free and adaptive where DeviceGradientAscent is local.  Points outside the box are projected onto it.
"""
import logging

import numpy as np

from robo_amd.maximizers.random_sampling import BaseMaximizer

logger = logging.getLogger(__name__)


class CMAES(BaseMaximizer):

    def __init__(self, objective_function, lower, upper, verbose=True, restarts=0, n_func_evals=1000, rng=None,
                 n_samples=65536, popsize=None, sigma0=0.25):
        if lower.shape[0] == 1:
            raise RuntimeError("CMAES does not works in a one dimensional function space")
        super(CMAES, self).__init__(objective_function, lower, upper, rng)
        self.restarts = int(restarts)
        self.verbose = verbose
        self.n_func_evals = int(n_func_evals)
        self.n_samples = int(n_samples)
        self.popsize = popsize
        self.sigma0 = float(sigma0)

    def maximize(self):
        from robo_amd import _lib
        from robo_amd.acquisition_functions.base_acquisition import ClosedFormAcquisition
        acq = self.objective_func
        inner = getattr(acq, "acquisition_func", acq)
        if not isinstance(inner, ClosedFormAcquisition):
            raise TypeError("CMAES needs EI, LogEI, PI or LCB (or MarginalizationGPMCMC over one of them): %s has no "
                            "moments-only value on the device" % type(inner).__name__)
        model = acq.model
        sub = model.models[0] if hasattr(model, "models") and len(model.models) > 0 else model
        from robo_amd.models.fabolas_gp import FabolasGP      # (its fidelity column is not a box coordinate)
        if not getattr(sub, "normalize_input", False) or not hasattr(sub, "gp") or isinstance(sub, FabolasGP):
            raise TypeError("CMAES needs a robo_amd GaussianProcess model with normalize_input=True")
        if getattr(model, "devices", None) or getattr(sub, "devices", None):
            raise NotImplementedError("CMAES runs on one device")
        if not sub.is_trained:
            raise Exception('Model has to be trained first!')
        sub._materialise()
        lower, upper = np.asarray(sub.lower, dtype=np.float64), np.asarray(sub.upper, dtype=np.float64)
        inc = np.asarray(model.get_incumbent()[0], dtype=np.float64)
        seed = int(self.rng.randint(0, 2 ** 31 - 1))
        cand = _lib.Candidates(sub.gp.ctx, m=self.n_samples, seed=seed, n_uniform=int(self.n_samples * .7),
                               loc=(inc - lower) / (upper - lower), scale=0.1 / (upper - lower))
        popsize = _lib.cmaes_default_popsize(len(lower)) if self.popsize is None else int(self.popsize)
        try:
            x = acq.cmaes(cand, n_instances=min(self.restarts + 1, self.n_samples), popsize=popsize,
                          n_generations=max(1, self.n_func_evals // popsize), sigma0=self.sigma0,
                          seed=int(self.rng.randint(0, 2 ** 31 - 1)))
        finally:
            cand.close()
        if self.verbose:
            res = acq.last_cmaes
            logger.info("CMAES: value %.6g from instance %d, flags %d", res.value, res.instance, res.flags)
        return x
