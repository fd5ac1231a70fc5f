"""Acquisition maximisation by sampling on the device and refining the best candidates by gradient ascent there.

``DeviceGradientAscent`` draws :class:`DeviceRandomSampling`'s candidates (70 % uniform over the box, 30 %
N(incumbent, 0.1) clipped; Philox, seeded from the maximiser's rng), scores them with one fused acquisition call and lets
the ``n_starts`` best of them climb ``n_steps`` projected gradient steps in lock step without leaving the device
(robo_acq_refine_cand / robo_acq_refine_marginal_cand): the first maximiser here whose answer is not one of the
candidates.  Not in the reference, whose gradient-based maximiser (robo/maximizers/scipy_optimizer.py) runs L-BFGS-B with
finite differences from the host, one 1 x D acquisition call per function value.

A ``ConstrainedEI`` climbs on the constrained value (robo_cei_refine_cand), its candidates drawn around the feasible
incumbent.  A ``ThompsonSampling`` objective is refined on its paths instead (robo_paths_refine_cand): per path the best rows of the
best groups of candidates descend on the path itself, all in one launch; ``maximize_batch(q)`` -- which only such a
maximiser has -- returns the q paths' refined minimisers (``ThompsonSampling.select_batch(refine=True)``).
"""
import numpy as np

from robo_amd.maximizers.random_sampling import BaseMaximizer


class DeviceGradientAscent(BaseMaximizer):

    def __init__(self, objective_function, lower, upper, n_samples=65536, n_starts=256, n_steps=50, step0=0.05,
                 rng=None):
        super(DeviceGradientAscent, self).__init__(objective_function, lower, upper, rng)
        self.n_samples = int(n_samples)
        self.n_starts = int(n_starts)
        self.n_steps = int(n_steps)
        self.step0 = float(step0)
        from robo_amd.acquisition_functions.thompson_sampling import ThompsonSampling
        if isinstance(objective_function, ThompsonSampling):      # (every other objective keeps the solver's refusal of batches)
            self.maximize_batch = self._maximize_batch_paths

    def _maximize_batch_paths(self, q, **unused):
        """the q paths' refined minimisers from ONE candidate batch (the recipe of maximize()) -> (q, D)"""
        return self.maximize(q=int(q))

    def maximize(self, q=None):
        from robo_amd import _lib
        from robo_amd.acquisition_functions.base_acquisition import ClosedFormAcquisition
        from robo_amd.acquisition_functions.constrained_ei import ConstrainedEI
        from robo_amd.acquisition_functions.thompson_sampling import ThompsonSampling
        acq = self.objective_func
        inner = getattr(acq, "acquisition_func", acq)
        if not isinstance(inner, (ClosedFormAcquisition, ThompsonSampling, ConstrainedEI)):
            raise TypeError("DeviceGradientAscent needs EI, LogEI, PI or LCB (or MarginalizationGPMCMC over one of them), "
                            "ConstrainedEI or ThompsonSampling: %s has no gradient on the device" % type(inner).__name__)
        model = acq.model
        sub = model.models[0] if hasattr(model, "models") and len(model.models) > 0 else model
        if isinstance(inner, ConstrainedEI):       # the objective's context and box, the feasible incumbent (as
            sub = model.objective                  # DeviceRandomSampling draws for it); refine() checks the constraints' models
        from robo_amd.models.fabolas_gp import FabolasGP      # (its fidelity column is not a box coordinate)
        if not getattr(sub, "normalize_input", False) or not hasattr(sub, "gp") or isinstance(sub, FabolasGP):
            raise TypeError("DeviceGradientAscent needs a robo_amd GaussianProcess model with normalize_input=True")
        if getattr(model, "devices", None) or getattr(sub, "devices", None):
            raise NotImplementedError("DeviceGradientAscent runs on one device")
        if not sub.is_trained:
            raise Exception('Model has to be trained first!')
        sub._materialise()
        lower, upper = np.asarray(sub.lower, dtype=np.float64), np.asarray(sub.upper, dtype=np.float64)
        inc = np.asarray(model.get_incumbent()[0], dtype=np.float64)
        loc = (inc - lower) / (upper - lower)
        scale = 0.1 / (upper - lower)
        seed = int(self.rng.randint(0, 2 ** 31 - 1))
        cand = _lib.Candidates(sub.gp.ctx, m=self.n_samples, seed=seed, n_uniform=int(self.n_samples * .7), loc=loc,
                               scale=scale)
        try:
            if q is not None:
                return acq.select_batch(cand, q, refine=True, n_starts=min(self.n_starts, self.n_samples),
                                        n_steps=self.n_steps, step0=self.step0)
            return acq.refine(cand, n_starts=min(self.n_starts, self.n_samples), n_steps=self.n_steps, step0=self.step0)
        finally:
            cand.close()
