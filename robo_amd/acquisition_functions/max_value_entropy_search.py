"""Max-value entropy search (Wang & Jegelka, ICML 2017) for minimisation -- no counterpart in the reference.

The acquisition is the expected reduction of the entropy of the MINIMUM VALUE y*, not of its location: per model update K
values y*_k are drawn from a Gumbel distribution fitted to the quartiles of max_i(-f(x_i)) over a discretisation
{x_i} (independence approximation), then

    alpha(x) = (1/K) sum_k [ gamma phi(gamma) / (2 Phi(gamma)) - log Phi(gamma) ],   gamma = (mu(x) - y*_k) / sigma(x).

All arithmetic runs on the device (robo_amd/csrc/mes.hip; the rule is stated in include/robo_hip.h):

* ``compute(X)`` is the paper's form: one set of y* per ``update()``, drawn over ``n_grid`` uniform points of the box
  plus the training inputs (one ``predict`` + ``robo_mes_sample_min_moments``), then the element-wise half at X
  (``robo_mes_eval_moments``).  It works with every maximiser, the single-point ones included, and with any model that
  has ``predict``.
* ``argmax(X)`` is the fused call with X itself as the discretisation (``robo_mes_eval_cand``): sweep, quartile search,
  Gumbel fit, draws, values and argmax with one synchronisation and no value crossing PCIe.  Fresh draws per call.

Random numbers come from ``rng`` in a stated order: first the ``n_grid x D`` grid (compute only), then the K uniforms.
"""
import numpy as np

from robo_amd import _lib
from robo_amd.acquisition_functions.base_acquisition import (BaseAcquisitionFunction, host_points, refuse_multi_device,
                                                             staged_candidates)


def mes_uniforms(rng, shape):
    """uniforms in the OPEN interval (0, 1) from a legacy RandomState (random_sample() can return 0.0)"""
    u = rng.random_sample(shape)
    return np.clip(u, np.finfo(np.float64).tiny, 1.0 - np.finfo(np.float64).epsneg)


def mes_box(model):
    lower, upper = getattr(model, "lower", None), getattr(model, "upper", None)
    if lower is None or upper is None:
        raise ValueError("MES draws its discretisation from the box [model.lower, model.upper]: the model has none")
    return np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)


def mes_grid(model, rng, n_grid):
    """the discretisation y* is sampled over, in the caller's input space: n_grid uniform points of the box + the
    training inputs"""
    lower, upper = mes_box(model)
    G = lower + (upper - lower) * rng.random_sample((int(n_grid), lower.shape[0]))
    X = getattr(model, "X", None)
    if X is not None and np.ndim(X) == 2 and np.shape(X)[1] == lower.shape[0]:
        X = np.asarray(X, dtype=np.float64)
        if getattr(model, "normalize_input", False):
            X = lower + (upper - lower) * X
        G = np.concatenate((G, X), axis=0)
    return G


# why a ``devices=...`` model is refused (refuse_multi_device)
MES_ONE_DEVICE = "a shard-consistent y* needs a cross-device reduction of F, which is not implemented"


class MES(BaseAcquisitionFunction):

    # y* is sampled over the candidates a call sees: a rank's slice would give every rank its own acquisition, so the
    # sampling maximisers refuse shard=True for this class (maximizers/random_sampling.py _check_candidate_shard)
    candidate_shard = False

    def __init__(self, model, n_samples=10, n_grid=10000, clamp=True, rng=None):
        super(MES, self).__init__(model)
        if not 1 <= int(n_samples) <= _lib.MES_MAX_K:
            raise ValueError("MES: n_samples = %r outside 1 .. %d" % (n_samples, _lib.MES_MAX_K))
        self.n_samples = int(n_samples)
        self.n_grid = int(n_grid)
        self.clamp = bool(clamp)
        self.rng = np.random.RandomState(np.random.randint(0, 10000)) if rng is None else rng
        self._ystar = None
        self.last_max = None
        self.last_argmax = None
        self.last_ystar = None

    def update(self, model):
        self.model = model
        self._ystar = None

    def _is_native(self):
        return hasattr(self.model, "acquisition") and hasattr(self.model, "gp")

    def _ctx(self):
        if self._is_native():
            self.model._materialise()
            return self.model.gp.ctx
        return _lib.default_context()

    def _eta(self):
        return float(self.model.get_incumbent()[1]) if self.clamp else 0.0

    def _moments(self, X):
        m, v = self.model.predict(X)
        return np.asarray(m, dtype=np.float64).ravel(), np.asarray(v, dtype=np.float64).ravel()

    def sampled_minima(self):
        """the K values y* this update's compute() calls use (drawn on first use)"""
        if self._ystar is None:
            refuse_multi_device([self.model], "MES", MES_ONE_DEVICE)
            G = mes_grid(self.model, self.rng, self.n_grid)
            u = mes_uniforms(self.rng, self.n_samples)
            m, v = self._moments(G)
            self._ystar = _lib.mes_sample_min(self._ctx(), m, v, u, self.clamp, self._eta())
        return self._ystar

    def compute(self, X, derivative=False, **kwargs):
        if derivative:
            raise NotImplementedError("MES has no derivative")
        refuse_multi_device([self.model], "MES", MES_ONE_DEVICE)
        X = host_points(self.model, X, "MES.compute", box=mes_box)
        ystar = self.sampled_minima()
        m, v = self._moments(X)
        vals, mx, am, _ = _lib.mes_from_moments(self._ctx(), m, v, ystar)
        self.last_max, self.last_argmax, self.last_ystar = mx, am, ystar
        return vals

    def argmax(self, X):
        """Index of the best candidate of X ((M, D) in the caller's input space, or a device batch ``_lib.Candidates`` in
        the normalised one), X itself being the discretisation y* is sampled over; fresh draws from ``rng`` per call."""
        if isinstance(X, _lib.CandidateShards):
            raise NotImplementedError("MES.argmax runs on one device: candidate shards are not implemented")
        refuse_multi_device([self.model], "MES", MES_ONE_DEVICE)
        if not self._is_native():
            m, v = self._moments(np.asarray(X, dtype=np.float64))
            u = mes_uniforms(self.rng, self.n_samples)
            ystar = _lib.mes_sample_min(self._ctx(), m, v, u, self.clamp, self._eta())
            _, mx, am, _ = _lib.mes_from_moments(self._ctx(), m, v, ystar)
        else:
            model = self.model
            if not model.is_trained:
                raise Exception('Model has to be trained first!')
            model._materialise()
            with staged_candidates(model, X) as cand:
                u = mes_uniforms(self.rng, self.n_samples)
                res = model.gp.mes(self._eta(), cand, u, self.clamp, want_values=False)
            mx, am, ystar = res.max, res.argmax, res.ystar
        self.last_max, self.last_argmax, self.last_ystar = mx, am, ystar
        return int(am)

    def argmax_sharded(self, comm, X_slice, global_offset):
        raise NotImplementedError("MES has no candidate shard: a shard-consistent y* needs a cross-rank reduction of F, "
                                  "which is not implemented (use shard=False)")
