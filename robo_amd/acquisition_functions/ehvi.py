"""Expected hypervolume improvement over two, three or four objectives (Emmerich, Deutz & Klinkenberg 2011) for minimisation
-- no counterpart in the reference.

EI, PI, LogEI, MES and the knowledge gradient score a candidate against one objective.  EHVI scores it against two at once:
the expected gain in the hypervolume the observed Pareto front dominates inside a reference point, for two objectives
with independent posteriors.  With the front sorted by the first objective the region still open is a union of strips and

    EHVI(x) = sum_i [ g(a_{i+1}; mu1, s1) - g(a_i; mu1, s1) ] g(b_i; mu2, s2),    g(b; mu, s) = E[(b - y)^+],

All arithmetic runs on the device (robo_amd/csrc/ehvi.hip; the rule is stated in include/robo_hip.h):

* two native device models on one context, with one input box, use the fused call (``robo_ehvi_eval_cand``): both sweeps,
  the strip kernel and the argmax with one synchronisation;
* any other pair of models with ``predict`` supplies its moments and the strip kernel alone runs on them
  (``robo_ehvi_eval_moments``) -- a ``GaussianProcessMCMC`` enters with its mixture moments.

With three or four objectives the open region is a set of boxes (util.pareto.nondominated_boxes) and

    EHVI(x) = sum_b prod_k [ g(t_k[hi_bk]; mu_k, s_k) - g(t_k[lo_bk]; mu_k, s_k) ]

runs in robo_amd/csrc/ehvi_box.hip through ``robo_ehvi_box_eval_cand`` / ``robo_ehvi_box_eval_moments``, split between native
and other models in the same way.  Two objectives keep the strip calls.

The front is fixed per ``update()``: the non-dominated training targets of the models inside ``ref_point``.
"""
import numpy as np

from robo_amd import _lib
from robo_amd.acquisition_functions.base_acquisition import OneDeviceAcquisition, predicted_moments, same_box_natives
from robo_amd.util.pareto import (exclusive_contributions, exclusive_contributions_2d, nondominated_boxes, pareto_front,
                                  pareto_front_2d)


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
    """what an EHVI holds as its ``model``: the two to four objectives' models (``objectives``), the box of the first, the
    observed front (with more than two objectives also its ``bounds`` and ``boxes``), and an incumbent for the maximisers
    that draw around one"""

    def __init__(self, objectives, ref_point):
        objectives = list(objectives)
        if not 2 <= len(objectives) <= _lib.EHVI_BOX_MAX_OBJ:
            raise ValueError("EHVI takes two to %d models, one per objective (got %d)"
                             % (_lib.EHVI_BOX_MAX_OBJ, len(objectives)))
        self.objectives = objectives
        self.ref_point = np.array(ref_point, dtype=np.float64).reshape(len(objectives))
        if not np.all(np.isfinite(self.ref_point)):
            raise ValueError("EHVI: ref_point %r is not finite" % (ref_point,))
        self.Y = self.front = self.front_indices = self.bounds = self.boxes = None

    lower = property(lambda self: self.objectives[0].lower)
    upper = property(lambda self: self.objectives[0].upper)

    def observe(self):
        """the front of the models' training targets (nothing when a model holds no data yet)"""
        if any(getattr(m, "y", None) is None for m in self.objectives):
            self.Y = self.front = self.front_indices = self.bounds = self.boxes = None
            return
        ys = [_targets(m) for m in self.objectives]
        for y in ys[1:]:
            if ys[0].shape != y.shape:
                raise ValueError("EHVI: the models hold %d and %d observations; they must be the same points"
                                 % (ys[0].shape[0], y.shape[0]))
        self.Y = np.stack(ys, axis=1)
        if len(ys) > 2:
            self.front, self.front_indices = pareto_front(self.Y, self.ref_point)
            self.bounds, self.boxes = nondominated_boxes(self.front, self.ref_point)
            return
        self.front, self.front_indices = pareto_front_2d(self.Y, self.ref_point)
        if self.front.shape[0] > _lib.EHVI_MAX_FRONT:
            raise ValueError("EHVI: a front of %d points, the device takes %d" % (self.front.shape[0], _lib.EHVI_MAX_FRONT))

    def get_incumbent(self):
        """the observed front point that alone adds the most hypervolume (ties: the lowest index); with an empty front the
        observation with the lowest first objective  -> (x, (y1, .., yK))"""
        if self.Y is None:
            self.observe()
        if self.Y is None:
            raise Exception('Model has to be trained first!')
        if self.front.shape[0] > 0:
            contrib = (exclusive_contributions_2d if self.Y.shape[1] == 2 else exclusive_contributions)(self.front,
                                                                                                     self.ref_point)
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
        """the retrained models (a list, or the ObjectivePair this function holds): the front is recomputed from their
        training targets"""
        if isinstance(models, ObjectivePair):
            self.model = models
            self.model.ref_point = self.ref_point
        else:
            self.model = ObjectivePair(models, self.ref_point)
        self.model.observe()

    @property
    def front(self):
        """this update's front (P, K): sorted by the first objective (K = 2), in lexicographic order (K > 2)"""
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
        """(mean1, var1, mean2, var2, ..), (M,) each, from the models' predict()"""
        return tuple(a for pair in predicted_moments(self.model.objectives, X) for a in pair)

    def _from_moments(self, Xhost):
        front = self.front
        mom = self.moments(Xhost)
        if len(mom) == 4:
            return _lib.ehvi_from_moments(_lib.default_context(), *mom, front=front, ref=self.ref_point)[:3]
        return _lib.ehvi_box_from_moments(_lib.default_context(), np.stack(mom[0::2]), np.stack(mom[1::2]), self.model.bounds,
                                          self.model.boxes)[:3]

    def _fused(self, cand, want_values):
        front = self.front
        gps = [m.gp for m in self.model.objectives]
        if len(gps) == 2:
            res = gps[0].ehvi(gps[1], cand, front, self.ref_point, want_values=want_values)
        else:
            res = gps[0].ehvi_box(gps[1:], cand, self.model.bounds, self.model.boxes, want_values=want_values)
        return res.values, res.max, res.argmax
