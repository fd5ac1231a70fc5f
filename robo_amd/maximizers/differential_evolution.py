"""Differential evolution on the acquisition function -- robo/maximizers/differential_evolution.py:7-51, i.e.
``maximizer="differential_evolution"`` of the front ends (robo/fmin/bayesian_optimization.py:135-136,
robo/fmin/entropy_search.py:108-109): ``scipy.optimize.differential_evolution(-acq(clip(x)), box, maxiter=n_iters)`` with
SciPy's defaults (population 15 D, best1bin, immediate updating, L-BFGS-B polish; its random numbers come from the global
NumPy stream), infinite values mapped to ``sys.float_info.max`` (:27-34), the result clipped to the box (:51).

In that form every objective call evaluates ONE point (on the device: the matrix-vector form of the explicit-inverse
posterior, 0.05 ms per call at N = 4096).  ``batched=True`` (not in the reference) hands SciPy a vectorised objective
instead: a whole generation -- 15 D trial points -- is scored by ONE device call (SciPy then updates the population once per
generation, "deferred", so the search path differs from the reference's immediate updating; same algorithm family, same
stopping rule).

``device=True`` (not in the reference either) runs the whole maximisation on the device with ONE synchronisation
(robo_acq_de_cand / robo_acq_de_marginal_cand): ``n_instances`` independent best1bin populations of ``popsize`` members
(None: min(15 D, 16384 // D, 1024)) in lock step for ``n_iters`` generations with SciPy's defaults (F dithered in
(0.5, 1), cr 0.7, tol 0.01, atol 0, deferred updating).  The start members are :class:`CMAES`'s candidates (70 % uniform over
the box, 30 % N(incumbent, 0.1) clipped; Philox, seeded from the maximiser's rng).  There is NO polish step:
:class:`DeviceGradientAscent` is the local finisher.  EI, LogEI, PI or LCB (or MarginalizationGPMCMC over one of them) over a
robo_amd GaussianProcess with normalize_input=True, one device."""
import sys

import numpy as np
from scipy import optimize

from robo_amd.maximizers.random_sampling import BaseMaximizer


class DifferentialEvolution(BaseMaximizer):

    def __init__(self, objective_function, lower, upper, n_iters=20, rng=None, batched=False, device=False, n_instances=1,
                 popsize=None):
        self.n_iters = n_iters
        self.batched = batched
        self.device = device
        self.n_instances = int(n_instances)
        self.popsize = popsize
        super(DifferentialEvolution, self).__init__(objective_function, lower, upper, rng)

    def _score(self, points):
        """-acq at the rows of `points` (clipped to the box), +inf/-inf -> the largest float (as the reference maps them)"""
        values = -np.asarray(self.objective_func(np.clip(points, self.lower, self.upper)), dtype=np.float64).reshape(-1)
        values[np.isinf(values)] = sys.float_info.max
        return values

    def _maximize_on_device(self):
        from robo_amd import _lib
        from robo_amd.acquisition_functions.base_acquisition import ClosedFormAcquisition
        acq = self.objective_func
        inner = getattr(acq, "acquisition_func", acq)
        if not isinstance(inner, ClosedFormAcquisition):
            raise TypeError("DifferentialEvolution(device=True) needs EI, LogEI, PI or LCB (or MarginalizationGPMCMC over one "
                            "of them): %s has no moments-only value on the device" % type(inner).__name__)
        model = acq.model
        sub = model.models[0] if hasattr(model, "models") and len(model.models) > 0 else model
        from robo_amd.models.fabolas_gp import FabolasGP      # (its fidelity column is not a box coordinate)
        if not getattr(sub, "normalize_input", False) or not hasattr(sub, "gp") or isinstance(sub, FabolasGP):
            raise TypeError("DifferentialEvolution(device=True) needs a robo_amd GaussianProcess model with normalize_input=True")
        if getattr(model, "devices", None) or getattr(sub, "devices", None):
            raise NotImplementedError("DifferentialEvolution(device=True) runs on one device")
        if not sub.is_trained:
            raise Exception('Model has to be trained first!')
        sub._materialise()
        lower, upper = np.asarray(sub.lower, dtype=np.float64), np.asarray(sub.upper, dtype=np.float64)
        inc = np.asarray(model.get_incumbent()[0], dtype=np.float64)
        popsize = _lib.de_default_popsize(len(lower)) if self.popsize is None else int(self.popsize)
        m = self.n_instances * popsize
        cand = _lib.Candidates(sub.gp.ctx, m=m, seed=int(self.rng.randint(0, 2 ** 31 - 1)), n_uniform=int(m * .7),
                               loc=(inc - lower) / (upper - lower), scale=0.1 / (upper - lower))
        try:
            return acq.de(cand, n_instances=self.n_instances, popsize=popsize, n_generations=int(self.n_iters),
                          seed=int(self.rng.randint(0, 2 ** 31 - 1)))
        finally:
            cand.close()

    def maximize(self):
        if self.device:
            return self._maximize_on_device()
        box = list(zip(self.lower, self.upper))
        if self.batched:
            # SciPy passes a (D, S) array and expects (S,) values
            found = optimize.differential_evolution(lambda pop: self._score(np.atleast_2d(pop.T)), box, maxiter=self.n_iters,
                                                    vectorized=True, updating="deferred")
        else:
            found = optimize.differential_evolution(lambda x: self._score(x[None, :]), box, maxiter=self.n_iters)
        return np.clip(found["x"], self.lower, self.upper)
