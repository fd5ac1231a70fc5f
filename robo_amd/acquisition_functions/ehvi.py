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
from robo_amd.acquisition_functions.base_acquisition import OneDeviceAcquisition, predicted_moments, same_box_natives
from robo_amd.util.pareto import exclusive_contributions_2d, pareto_front_2d


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


class EHVI(OneDeviceAcquisition):

    def __init__(self, models, ref_point):
        pair = models if isinstance(models, ObjectivePair) else ObjectivePair(models, ref_point)
        super(EHVI, self).__init__(pair)
        self.ref_point = pair.ref_point
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

    def _models(self):
        return self.model.objectives

    def _is_native(self):
        return same_box_natives(self.model.objectives)

    def moments(self, X):
        """(mean1, var1, mean2, var2), (M,) each, from the two models' predict()"""
        (mean1, var1), (mean2, var2) = predicted_moments(self.model.objectives, X)
        return mean1, var1, mean2, var2

    def _from_moments(self, Xhost):
        front = self.front
        return _lib.ehvi_from_moments(_lib.default_context(), *self.moments(Xhost), front=front, ref=self.ref_point)[:3]

    def _fused(self, cand, want_values):
        m1, m2 = self.model.objectives
        res = m1.gp.ehvi(m2.gp, cand, self.front, self.ref_point, want_values=want_values)
        return res.values, res.max, res.argmax
