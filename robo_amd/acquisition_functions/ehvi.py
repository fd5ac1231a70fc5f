"""Two-objective expected hypervolume improvement (Emmerich, Deutz & Klinkenberg 2011) for minimisation -- no counterpart
in the reference.

EI, PI, LogEI, MES and the knowledge gradient score a candidate against one objective.  EHVI scores it against two at once:
the expected gain in the hypervolume the observed Pareto front dominates inside a reference point, for two objectives
with independent posteriors.  With the front sorted by the first objective the region still open is a union of strips and

    EHVI(x) = sum_i [ g(a_{i+1}; mu1, s1) - g(a_i; mu1, s1) ] g(b_i; mu2, s2),    g(b; mu, s) = E[(b - y)^+],

All arithmetic runs on the device (robo_amd/csrc/ehvi.hip; the rule is stated in include/robo_hip.h):

* two native device models on one context, with one input box, use the fused call (``robo_ehvi_eval_cand``): both sweeps,
  the strip kernel and the argmax with one synchronisation;
* any other pair of models with ``predict`` supplies its moments and the strip kernel alone runs on them
  (``robo_ehvi_eval_moments``) -- a ``GaussianProcessMCMC`` enters with its mixture moments.

The front is fixed per ``update()``: the non-dominated training targets of the two models inside ``ref_point``.
"""
import numpy as np

from robo_amd import _lib
from robo_amd.acquisition_functions.base_acquisition import BaseAcquisitionFunction
from robo_amd.util.pareto import exclusive_contributions_2d, pareto_front_2d

_MOMENT_ROWS = 512          # candidates per predict() call of the moments path


def _targets(model):
    """the model's training targets in the scale predict() returns"""
    y = getattr(model, "y", None)
    if y is None:
        raise ValueError("EHVI takes its front from the models' training targets: %s has none" % type(model).__name__)
    y = np.asarray(y, dtype=np.float64).ravel()
    if getattr(model, "normalize_output", False):
        y = y * model.y_std + model.y_mean
    return y


def _inputs(model):
    """the model's training inputs in the caller's input space"""
    X = np.asarray(model.X, dtype=np.float64)
    if getattr(model, "normalize_input", False) and not hasattr(model, "normalize"):
        lower, upper = np.asarray(model.lower, dtype=np.float64), np.asarray(model.upper, dtype=np.float64)
        X = lower + (upper - lower) * X
    return X


class ObjectivePair(object):
    """what an EHVI holds as its ``model``: the two objectives' models (``objectives``), the box of the first, the observed
    front, and an incumbent for the maximisers that draw around one"""

    def __init__(self, objectives, ref_point):
        objectives = list(objectives)
        if len(objectives) != 2:
            raise ValueError("EHVI takes a pair of models, one per objective (got %d)" % len(objectives))
        self.objectives = objectives
        self.ref_point = np.array(ref_point, dtype=np.float64).reshape(2)
        if not np.all(np.isfinite(self.ref_point)):
            raise ValueError("EHVI: ref_point %r is not finite" % (ref_point,))
        self.Y = self.front = self.front_indices = None

    lower = property(lambda self: self.objectives[0].lower)
    upper = property(lambda self: self.objectives[0].upper)

    def observe(self):
        """the front of the two models' training targets (nothing when a model holds no data yet)"""
        if any(getattr(m, "y", None) is None for m in self.objectives):
            self.Y = self.front = self.front_indices = None
            return
        y1, y2 = _targets(self.objectives[0]), _targets(self.objectives[1])
        if y1.shape != y2.shape:
            raise ValueError("EHVI: the two models hold %d and %d observations; they must be the same points"
                             % (y1.shape[0], y2.shape[0]))
        self.Y = np.stack((y1, y2), axis=1)
        self.front, self.front_indices = pareto_front_2d(self.Y, self.ref_point)
        if self.front.shape[0] > _lib.EHVI_MAX_FRONT:
            raise ValueError("EHVI: a front of %d points, the device takes %d" % (self.front.shape[0], _lib.EHVI_MAX_FRONT))

    def get_incumbent(self):
        """the observed front point that alone adds the most hypervolume (ties: the lowest index); with an empty front the
        observation with the lowest first objective  -> (x, (y1, y2))"""
        if self.Y is None:
            self.observe()
        if self.Y is None:
            raise Exception('Model has to be trained first!')
        if self.front.shape[0] > 0:
            contrib = exclusive_contributions_2d(self.front, self.ref_point)
            j = int(np.min(self.front_indices[contrib == contrib.max()]))
        else:
            j = int(np.argmin(self.Y[:, 0]))
        return _inputs(self.objectives[0])[j], self.Y[j]


class EHVI(BaseAcquisitionFunction):

    # one device, one front: no candidate shard (maximizers/random_sampling.py _check_candidate_shard)
    candidate_shard = False

    def __init__(self, models, ref_point):
        pair = models if isinstance(models, ObjectivePair) else ObjectivePair(models, ref_point)
        super(EHVI, self).__init__(pair)
        self.ref_point = pair.ref_point
        self.last_max = None
        self.last_argmax = None
        pair.observe()

    def update(self, models):
        """the two retrained models (a pair, or the ObjectivePair this function holds): the front is recomputed from their
        training targets"""
        if isinstance(models, ObjectivePair):
            self.model = models
            self.model.ref_point = self.ref_point
        else:
            self.model = ObjectivePair(models, self.ref_point)
        self.model.observe()

    @property
    def front(self):
        """this update's front (P, 2), sorted by the first objective"""
        if self.model.front is None:
            self.model.observe()
        if self.model.front is None:
            raise Exception('Model has to be trained first!')
        return self.model.front

    def _refuse_sharded(self):
        for m in self.model.objectives:
            if getattr(m, "devices", None):
                raise NotImplementedError("EHVI runs on one device: multi-device and sharded forms are not implemented "
                                          "(devices=%r)" % (m.devices,))

    def _is_native(self):
        """two device GPs that take the same normalised candidates: one context after materialising, one box"""
        m1, m2 = self.model.objectives
        for m in (m1, m2):
            if not (hasattr(m, "acquisition") and hasattr(m, "gp")) or hasattr(m, "normalize"):
                return False
        if bool(m1.normalize_input) != bool(m2.normalize_input):
            return False
        if m1.normalize_input and not (np.array_equal(m1.lower, m2.lower) and np.array_equal(m1.upper, m2.upper)):
            return False
        for m in (m1, m2):
            if not m.is_trained:
                raise Exception('Model has to be trained first!')
            m._materialise()
        return m1.gp.ctx is m2.gp.ctx

    def _host_points(self, X):
        """an array as it is; a device batch (normalised box) in the caller's input space, under the condition the
        knowledge gradient states"""
        if not isinstance(X, _lib.Candidates):
            return np.asarray(X, dtype=np.float64)
        m = self.model.objectives[0]
        if not getattr(m, "normalize_input", False) or hasattr(m, "normalize") or m.lower is None or m.upper is None:
            raise TypeError("EHVI on a device candidate batch needs models with normalize_input=True whose input space is "
                            "the normalised box (not a Fabolas model); pass the points as an array instead")
        lower, upper = np.asarray(m.lower, dtype=np.float64), np.asarray(m.upper, dtype=np.float64)
        return lower + (upper - lower) * X.points()

    def moments(self, X):
        """(mean1, var1, mean2, var2), (M,) each, from the two models' predict(), _MOMENT_ROWS candidates per call"""
        out = [[], [], [], []]
        for r0 in range(0, X.shape[0], _MOMENT_ROWS):
            rows = X[r0:r0 + _MOMENT_ROWS]
            for o, m in enumerate(self.model.objectives):
                mu, var = m.predict(rows)[:2]
                out[2 * o].append(np.asarray(mu, dtype=np.float64).ravel())
                out[2 * o + 1].append(np.asarray(var, dtype=np.float64).ravel())
        return tuple(np.concatenate(a) for a in out)

    def _evaluate(self, X, want_values):
        self._refuse_sharded()
        if isinstance(X, _lib.CandidateShards):
            raise NotImplementedError("EHVI runs on one device: candidate shards are not implemented")
        front = self.front
        if not self._is_native():
            vals, mx, am, _ = _lib.ehvi_from_moments(_lib.default_context(), *self.moments(self._host_points(X)), front=front,
                                                     ref=self.ref_point)
        else:
            m1, m2 = self.model.objectives
            cand = X
            if isinstance(X, _lib.Candidates):
                if not m1.normalize_input:
                    self._host_points(X)                                         # raises the TypeError
            else:
                cand = _lib.Candidates(m1.gp.ctx, m1._normalised(np.asarray(X, dtype=np.float64)))
            try:
                res = m1.gp.ehvi(m2.gp, cand, front, self.ref_point, want_values=want_values)
            finally:
                if cand is not X:
                    cand.close()
            vals, mx, am = res.values, res.max, res.argmax
        self.last_max, self.last_argmax = mx, int(am)
        return vals

    def compute(self, X, derivative=False, **kwargs):
        if derivative:
            raise NotImplementedError("EHVI has no derivative")
        return self._evaluate(X, True)

    def argmax(self, X):
        """Index of the best candidate of X ((M, D) in the caller's input space, or a device batch ``_lib.Candidates`` in
        the normalised one): on the fused path only the maximiser comes back."""
        self._evaluate(X, False)
        return int(self.last_argmax)

    def argmax_sharded(self, comm, X_slice, global_offset):
        raise NotImplementedError("EHVI has no candidate shard: multi-device and sharded forms are not implemented (use "
                                  "shard=False)")
