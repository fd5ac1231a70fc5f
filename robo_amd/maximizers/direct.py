"""Acquisition maximisation by DIRECT on the device.

``Direct`` has the signature of robo/maximizers/direct.py (which drives the ``DIRECT`` package from the host, one 1 x D
acquisition call per function value); everything else sits behind the reference's parameters.  Jones, Perttunen and
Stuckman's DIviding RECTangles in its original form runs over the model's normalised box without leaving the device
(robo_acq_direct / robo_acq_direct_marginal): ``n_func_evals`` values in at most ``n_iters`` iterations, every iteration's
new points as one posterior batch of ``batch`` rows.  The only deterministic global maximiser of the family: it takes no
draws and no starting points (``rng`` is accepted for the family's signature and never used), so the same model gives the
same proposal.  One dimension is fine.
"""
import logging

from robo_amd.maximizers.random_sampling import BaseMaximizer

logger = logging.getLogger(__name__)


class Direct(BaseMaximizer):

    def __init__(self, objective_function, lower, upper, n_func_evals=400, n_iters=200, verbose=True, eps=1e-4, batch=None,
                 rng=None):
        super(Direct, self).__init__(objective_function, lower, upper, rng)
        self.n_func_evals = int(n_func_evals)
        self.n_iters = int(n_iters)
        self.verbose = verbose
        self.eps = float(eps)
        self.batch = batch

    def maximize(self):
        from robo_amd.acquisition_functions.base_acquisition import ClosedFormAcquisition
        acq = self.objective_func
        inner = getattr(acq, "acquisition_func", acq)
        if not isinstance(inner, ClosedFormAcquisition):
            raise TypeError("Direct needs EI, LogEI, PI or LCB (or MarginalizationGPMCMC over one of them): %s has no "
                            "moments-only value on the device" % type(inner).__name__)
        model = acq.model
        sub = model.models[0] if hasattr(model, "models") and len(model.models) > 0 else model
        from robo_amd.models.fabolas_gp import FabolasGP      # (its fidelity column is not a box coordinate)
        if not getattr(sub, "normalize_input", False) or not hasattr(sub, "gp") or isinstance(sub, FabolasGP):
            raise TypeError("Direct needs a robo_amd GaussianProcess model with normalize_input=True")
        if getattr(model, "devices", None) or getattr(sub, "devices", None):
            raise NotImplementedError("Direct runs on one device")
        if not sub.is_trained:
            raise Exception('Model has to be trained first!')
        x = acq.direct(self.n_func_evals, self.n_iters, eps=self.eps, batch=self.batch)
        if self.verbose:
            res = acq.last_direct
            logger.info("Direct: value %.6g after %d values in %d iterations, flags %#x", res.value, res.evals, res.iters,
                        res.flags)
        return x
