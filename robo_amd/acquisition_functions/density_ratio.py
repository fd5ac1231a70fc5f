"""TPE's acquisition: log l(x) - log g(x) of a models.TPE, monotone in EI (Bergstra et al. 2011).  Both densities, the ratio
and its argmax over a candidate batch are one fused device call (robo_kde_ratio_eval_cand); ``argmax`` is the form the
random-sampling maximisers take, with which only the winner's index comes back."""
import numpy as np

from robo_amd.acquisition_functions.base_acquisition import BaseAcquisitionFunction


class DensityRatio(BaseAcquisitionFunction):

    candidate_shard = False       # one device (maximizers/random_sampling.py _check_candidate_shard)

    def __init__(self, model):
        if not hasattr(model, "ratio"):
            raise TypeError("DensityRatio needs a model with a density ratio (models.TPE), got %s" % type(model).__name__)
        super(DensityRatio, self).__init__(model)
        self.last_max = self.last_argmax = self.last_flags = None

    def compute(self, X, derivative=False, **kwargs):
        if derivative:
            raise NotImplementedError("DensityRatio has no derivative")
        vals, self.last_max, self.last_argmax, self.last_flags = self.model.ratio(np.atleast_2d(X))
        return vals

    def argmax(self, X):
        """index of the best candidate (np.argmax: first index, NaN maximal) without copying the values back"""
        _, self.last_max, self.last_argmax, self.last_flags = self.model.ratio(np.atleast_2d(X), want_values=False)
        return int(self.last_argmax)
