"""Constrained expected improvement (Schonlau, Welch & Jones 1998; Gardner et al. 2014; Gelbart, Snoek & Adams 2014) for
minimisation under black-box constraints -- no counterpart in the reference.

Every evaluation returns an objective value and C constraint values; constraint k holds when c_k(x) <= t_k.  One model per
output, independent posteriors:

    CEI(x) = EI(x; eta) * prod_k P(c_k(x) <= t_k),        eta = the lowest FEASIBLE observed objective,

and while no feasible point has been observed the probability of feasibility alone.  ``log=True`` is the same rule in logs:
LogEI + sum_k log P, which stays finite where the product has long underflowed.

All arithmetic runs on the device (robo_amd/csrc/cei.hip; the rule is stated in include/robo_hip.h):

* native device models on one context, with one input box, use the fused call (``robo_cei_eval_cand``): the C + 1 sweeps,
  the fold kernel and the argmax with one synchronisation;
* any other set of models with ``predict`` supplies its moments and the fold kernel alone runs on them
  (``robo_cei_eval_moments``) -- a ``GaussianProcessMCMC`` enters with its mixture moments.

The incumbent is fixed per ``update()``, from the models' training targets.
"""
import numpy as np

from robo_amd import _lib
from robo_amd.acquisition_functions.base_acquisition import BaseAcquisitionFunction
from robo_amd.acquisition_functions.ehvi import _inputs, _targets

_MOMENT_ROWS = 512          # candidates per predict() call of the moments path


def _observed(C, thresholds):
    """observed constraint values as (n, C) (with no constraint at all the array must say how many points: (n, 0))"""
    C, k = np.asarray(C, dtype=np.float64), np.asarray(thresholds).reshape(-1).shape[0]
    return C if C.ndim == 2 and C.shape[1] == k else C.reshape(-1, k)


def feasible_mask(C, thresholds):
    """observed constraint values (n, C) against thresholds (C,) -> (n,) bool; a value ON its threshold is feasible"""
    return np.all(_observed(C, thresholds) <= np.asarray(thresholds, dtype=np.float64).reshape(1, -1), axis=1)


def feasible_incumbent(y, C, thresholds):
    """index of the lowest objective among the feasible observations (ties: the lowest index), or None"""
    ok = feasible_mask(C, thresholds)
    if not ok.any():
        return None
    return int(np.argmin(np.where(ok, np.asarray(y, dtype=np.float64), np.inf)))


def least_violation(C, thresholds):
    """index of the observation whose largest violation max_k (c_k - t_k) is smallest (ties: the lowest index)"""
    C = _observed(C, thresholds)
    if C.shape[1] == 0:
        return 0
    return int(np.argmin(np.max(C - np.asarray(thresholds, dtype=np.float64).reshape(1, -1), axis=1)))


class ConstrainedModels(object):
    """what a ConstrainedEI holds as its ``model``: the objective's model (``objective``), the constraints' (``constraints``),
    the thresholds, the box of the objective, and the feasible incumbent of the observations"""

    def __init__(self, objective, constraints, thresholds):
        self.objective = objective
        self.constraints = list(constraints)
        self.thresholds = np.array(thresholds, dtype=np.float64).reshape(-1)
        if self.thresholds.shape[0] != len(self.constraints):
            raise ValueError("ConstrainedEI: %d thresholds for %d constraint models"
                             % (self.thresholds.shape[0], len(self.constraints)))
        if len(self.constraints) > _lib.CEI_MAX_CONSTRAINTS:
            raise ValueError("ConstrainedEI: %d constraints, the device takes %d"
                             % (len(self.constraints), _lib.CEI_MAX_CONSTRAINTS))
        if not np.all(np.isfinite(self.thresholds)):
            raise ValueError("ConstrainedEI: thresholds %r are not finite" % (thresholds,))
        self.y = self.C = self.feasible = self.incumbent_index = self.eta = None

    lower = property(lambda self: self.objective.lower)
    upper = property(lambda self: self.objective.upper)
    all_models = property(lambda self: [self.objective] + self.constraints)

    def observe(self):
        """the feasible incumbent of the models' training targets (nothing when a model holds no data yet): ``eta`` is the
        lowest observed objective among the points whose constraint values all satisfy their thresholds, or None"""
        if any(getattr(m, "y", None) is None for m in self.all_models):
            self.y = self.C = self.feasible = self.incumbent_index = self.eta = None
            return
        self.y = _targets(self.objective)
        cols = [_targets(m) for m in self.constraints]
        for c in cols:
            if c.shape != self.y.shape:
                raise ValueError("ConstrainedEI: the models hold %d and %d observations; they must be the same points"
                                 % (self.y.shape[0], c.shape[0]))
        self.C = np.stack(cols, axis=1) if cols else np.zeros((self.y.shape[0], 0))
        self.feasible = feasible_mask(self.C, self.thresholds)
        self.incumbent_index = feasible_incumbent(self.y, self.C, self.thresholds)
        self.eta = None if self.incumbent_index is None else float(self.y[self.incumbent_index])

    def get_incumbent(self):
        """the feasible observation with the lowest objective; without a feasible one the observation with the smallest
        largest violation -> (x, y)"""
        if self.y is None:
            self.observe()
        if self.y is None:
            raise Exception('Model has to be trained first!')
        j = self.incumbent_index if self.incumbent_index is not None else least_violation(self.C, self.thresholds)
        return _inputs(self.objective)[j], self.y[j]


class ConstrainedEI(BaseAcquisitionFunction):

    # one device: no candidate shard (maximizers/random_sampling.py _check_candidate_shard)
    candidate_shard = False

    def __init__(self, models, thresholds, par=0.0, log=False):
        """models: a ConstrainedModels, or a sequence (objective model, constraint model 1, .. constraint model C)"""
        if not isinstance(models, ConstrainedModels):
            models = list(models)
            if len(models) < 1:
                raise ValueError("ConstrainedEI takes the objective's model followed by one model per constraint")
            models = ConstrainedModels(models[0], models[1:], thresholds)
        super(ConstrainedEI, self).__init__(models)
        self.thresholds = models.thresholds
        self.par = par
        self.log = bool(log)
        self.last_max = None
        self.last_argmax = None
        models.observe()

    kind = property(lambda self: "log_ei" if self.log else "ei")

    def update(self, models):
        """the retrained models (a sequence as the constructor takes it, or the ConstrainedModels this function holds): the
        feasible incumbent is recomputed from their training targets"""
        if isinstance(models, ConstrainedModels):
            self.model = models
            self.model.thresholds = self.thresholds
        else:
            models = list(models)
            self.model = ConstrainedModels(models[0], models[1:], self.thresholds)
        self.model.observe()

    @property
    def eta(self):
        """this update's feasible incumbent value, or None while no observation is feasible"""
        if self.model.y is None:
            self.model.observe()
        if self.model.y is None:
            raise Exception('Model has to be trained first!')
        return self.model.eta

    def _refuse_sharded(self):
        for m in self.model.all_models:
            if getattr(m, "devices", None):
                raise NotImplementedError("ConstrainedEI runs on one device: multi-device and sharded forms are not "
                                          "implemented (devices=%r)" % (m.devices,))

    def _is_native(self):
        """device GPs that take the same normalised candidates: one context after materialising, one box"""
        ms = self.model.all_models
        for m in ms:
            if not (hasattr(m, "acquisition") and hasattr(m, "gp")) or hasattr(m, "normalize"):
                return False
        first = ms[0]
        for m in ms[1:]:
            if bool(m.normalize_input) != bool(first.normalize_input):
                return False
            if first.normalize_input and not (np.array_equal(first.lower, m.lower) and np.array_equal(first.upper, m.upper)):
                return False
        for m in ms:
            if not m.is_trained:
                raise Exception('Model has to be trained first!')
            m._materialise()
        return all(m.gp.ctx is first.gp.ctx for m in ms)

    def _host_points(self, X):
        """an array as it is; a device batch (normalised box) in the caller's input space, under the condition EHVI states"""
        if not isinstance(X, _lib.Candidates):
            return np.asarray(X, dtype=np.float64)
        m = self.model.objective
        if not getattr(m, "normalize_input", False) or hasattr(m, "normalize") or m.lower is None or m.upper is None:
            raise TypeError("ConstrainedEI on a device candidate batch needs models with normalize_input=True whose input "
                            "space is the normalised box (not a Fabolas model); pass the points as an array instead")
        lower, upper = np.asarray(m.lower, dtype=np.float64), np.asarray(m.upper, dtype=np.float64)
        return lower + (upper - lower) * X.points()

    def moments(self, X):
        """(mean0, var0, means, vars): (M,), (M,), (C, M), (C, M) from the models' predict(), _MOMENT_ROWS candidates per call"""
        ms = self.model.all_models
        mu, var = [[] for _ in ms], [[] for _ in ms]
        for r0 in range(0, X.shape[0], _MOMENT_ROWS):
            rows = X[r0:r0 + _MOMENT_ROWS]
            for o, m in enumerate(ms):
                a, b = m.predict(rows)[:2]
                mu[o].append(np.asarray(a, dtype=np.float64).ravel())
                var[o].append(np.asarray(b, dtype=np.float64).ravel())
        mu, var = [np.concatenate(a) for a in mu], [np.concatenate(a) for a in var]
        M = mu[0].shape[0]
        return mu[0], var[0], np.array(mu[1:]).reshape(len(ms) - 1, M), np.array(var[1:]).reshape(len(ms) - 1, M)

    def _evaluate(self, X, want_values, feasibility_only=False):
        """-> (values or None, max, argmax) of the function itself, or of the probability of feasibility alone"""
        self._refuse_sharded()
        if isinstance(X, _lib.CandidateShards):
            raise NotImplementedError("ConstrainedEI runs on one device: candidate shards are not implemented")
        kind, eta = ("ei", None) if feasibility_only else (self.kind, self.eta)
        if not self._is_native():
            vals, mx, am, _ = _lib.cei_from_moments(_lib.default_context(), *self.moments(self._host_points(X)),
                                                    thresholds=self.thresholds, kind=kind, par=self.par, eta=eta)
        else:
            obj = self.model.objective
            cand = X
            if isinstance(X, _lib.Candidates):
                if not obj.normalize_input:
                    self._host_points(X)                                         # raises the TypeError
            else:
                cand = _lib.Candidates(obj.gp.ctx, obj._normalised(np.asarray(X, dtype=np.float64)))
            try:
                res = obj.gp.cei([m.gp for m in self.model.constraints], cand, self.thresholds, kind, self.par, eta,
                                 want_values=want_values)
            finally:
                if cand is not X:
                    cand.close()
            vals, mx, am = res.values, res.max, res.argmax
        return vals, mx, int(am)

    def compute(self, X, derivative=False, **kwargs):
        if derivative:
            raise NotImplementedError("ConstrainedEI has no derivative")
        vals, self.last_max, self.last_argmax = self._evaluate(X, True)
        return vals

    def argmax(self, X):
        """Index of the best candidate of X ((M, D) in the caller's input space, or a device batch ``_lib.Candidates`` in
        the normalised one): on the fused path only the maximiser comes back."""
        _, self.last_max, self.last_argmax = self._evaluate(X, False)
        return int(self.last_argmax)

    def probability_of_feasibility(self, X):
        """prod_k P(c_k(x) <= t_k) of every candidate, by the same device rule (the value the function takes while no
        observation is feasible); ``last_max`` / ``last_argmax`` are left alone"""
        return self._evaluate(X, True, feasibility_only=True)[0]

    def argmax_sharded(self, comm, X_slice, global_offset):
        raise NotImplementedError("ConstrainedEI has no candidate shard: multi-device and sharded forms are not implemented "
                                  "(use shard=False)")
