"""Knowledge gradient over a discretisation (Frazier, Powell & Dayanik 2009) for minimisation -- no counterpart in the
reference.

EI, PI and LogEI score a candidate against the incumbent observation; the knowledge gradient scores what a user of a
noisy objective wants: how much the minimum of the posterior MEAN over a discretisation A = {z_j} is expected to drop
after one more noisy observation at x,

    KG(x) = min_j mu(z_j) - E_Z[ min_j (mu(z_j) + b_j(x) Z) ],   b_j(x) = cov(x, z_j) / sqrt(var(x) + sn2),

with x itself as one more line (``include_self``).  All arithmetic runs on the device (robo_amd/csrc/kg.hip; the rule is
stated in include/robo_hip.h):

* a native device model uses the fused call (``robo_kg_eval_cand``): sweep, the discretisation's posterior, signed
  cross-covariances, the envelope kernel and the argmax with one synchronisation;
* any other model with ``predict`` and ``predict(full_cov=True)`` supplies its moments and the envelope kernel alone
  runs on them (``robo_kg_eval_moments``).

The discretisation is fixed per ``update()``: the caller's ``discretisation`` (nb, D) as given, or the ``n_disc`` points of
lowest posterior mean (ties by index) among ``n_grid`` uniform points of the box plus the training inputs -- one
``predict`` call.  Random numbers come from ``rng``: the ``n_grid x D`` grid, nothing else.
"""
from copy import deepcopy

import numpy as np

from robo_amd import _lib
from robo_amd.acquisition_functions.base_acquisition import BaseAcquisitionFunction
from robo_amd.acquisition_functions.max_value_entropy_search import mes_box, mes_grid

_MOMENT_ROWS = 512          # candidates per predict(full_cov=True) call of the moments path


def kg_refuse_sharded(model, who):
    if getattr(model, "devices", None):
        raise NotImplementedError("%s runs on one device: multi-device and sharded forms of the knowledge gradient are "
                                  "not implemented (devices=%r)" % (who, model.devices))


def kg_discretisation(model, rng, n_disc, n_grid, given=None):
    """the discretisation in the caller's input space: ``given`` (nb, D) as it is, or the n_disc points of lowest
    posterior mean among mes_grid's points (stable order: by mean, ties by index)"""
    if given is not None:
        Z = np.array(given, dtype=np.float64)
        if Z.ndim != 2 or not 1 <= Z.shape[0] <= _lib.KG_MAX_DISC:
            raise ValueError("KnowledgeGradient: discretisation must be (nb, D) with 1 <= nb <= %d, got %r"
                             % (_lib.KG_MAX_DISC, Z.shape))
        return Z
    G = mes_grid(model, rng, n_grid)
    mean = np.asarray(model.predict(G)[0], dtype=np.float64).ravel()
    return G[np.argsort(mean, kind="stable")[:n_disc]]


class KnowledgeGradient(BaseAcquisitionFunction):

    # the discretisation is chosen over the whole box: no candidate shard (maximizers/random_sampling.py
    # _check_candidate_shard)
    candidate_shard = False

    def __init__(self, model, n_disc=50, n_grid=10000, discretisation=None, include_self=True, rng=None):
        super(KnowledgeGradient, self).__init__(model)
        if not 1 <= int(n_disc) <= _lib.KG_MAX_DISC:
            raise ValueError("KnowledgeGradient: n_disc = %r outside 1 .. %d" % (n_disc, _lib.KG_MAX_DISC))
        self.n_disc = int(n_disc)
        self.n_grid = int(n_grid)
        self.discretisation = None if discretisation is None else kg_discretisation(None, None, 0, 0, discretisation)
        self.include_self = bool(include_self)
        self.rng = np.random.RandomState(np.random.randint(0, 10000)) if rng is None else rng
        self._disc = None            # this update's discretisation (caller's input space)
        self._rep = None             # ... as a device handle (native models): its solve is kept between calls
        self.last_max = None
        self.last_argmax = None

    def __deepcopy__(self, memo):
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for key, val in self.__dict__.items():
            new.__dict__[key] = None if key == "_rep" else deepcopy(val, memo)      # a device handle is not copied
        return new

    def _drop_rep(self):
        if self._rep is not None:
            self._rep.close()
            self._rep = None

    def update(self, model):
        self.model = model
        self._disc = None
        self._drop_rep()

    def _is_native(self):
        return hasattr(self.model, "acquisition") and hasattr(self.model, "gp")

    def _norm(self):
        return self.model.normalize if hasattr(self.model, "normalize") else self.model._normalised

    def discretisation_points(self):
        """this update's discretisation (nb, D) in the caller's input space (chosen on first use)"""
        if self._disc is None:
            kg_refuse_sharded(self.model, "KnowledgeGradient")
            self._disc = kg_discretisation(self.model, self.rng, self.n_disc, self.n_grid, self.discretisation)
            self._drop_rep()
        return self._disc

    def _rep_handle(self):
        Z = self.discretisation_points()
        if self._rep is None:
            self._rep = _lib.Candidates(self.model.gp.ctx, self._norm()(Z))
        return self._rep

    def _sn2(self):
        get = getattr(self.model, "get_noise", None)
        return float(get()) if get is not None else 0.0

    def _host_points(self, X):
        """an array as it is; a device batch (normalised box) in the caller's input space, under MES's condition"""
        if not isinstance(X, _lib.Candidates):
            return np.asarray(X, dtype=np.float64)
        if not getattr(self.model, "normalize_input", False) or hasattr(self.model, "normalize"):
            raise TypeError("KnowledgeGradient on a device candidate batch needs a model with normalize_input=True whose "
                            "input space is the normalised box (not a Fabolas model); pass the points as an array instead")
        lower, upper = mes_box(self.model)
        return lower + (upper - lower) * X.points()

    def moments(self, X):
        """(s (M, nb) signed-as-given covariances with the discretisation, v (M,), mean (M,), disc_mean (nb,)) from the
        model's predict(full_cov=True), _MOMENT_ROWS candidates per call"""
        Z = self.discretisation_points()
        nb = Z.shape[0]
        s, v, mean, disc = [], [], [], None
        for r0 in range(0, X.shape[0], _MOMENT_ROWS):
            rows = X[r0:r0 + _MOMENT_ROWS]
            mu, cov = self.model.predict(np.concatenate((rows, Z), axis=0), full_cov=True)
            mu, cov = np.asarray(mu, dtype=np.float64).ravel(), np.asarray(cov, dtype=np.float64)
            k = rows.shape[0]
            s.append(cov[:k, k:k + nb])
            v.append(np.diag(cov)[:k])
            mean.append(mu[:k])
            disc = mu[k:k + nb] if disc is None else disc
        return np.concatenate(s), np.concatenate(v), np.concatenate(mean), disc

    def _evaluate(self, X, want_values):
        kg_refuse_sharded(self.model, "KnowledgeGradient")
        if isinstance(X, _lib.CandidateShards):
            raise NotImplementedError("KnowledgeGradient runs on one device: candidate shards are not implemented")
        if not self._is_native():
            vals, mx, am, _ = _lib.kg_from_moments(_lib.default_context(), *self.moments(self._host_points(X)), sn2=self._sn2(),
                                                   include_self=self.include_self)
        else:
            model = self.model
            if not model.is_trained:
                raise Exception('Model has to be trained first!')
            model._materialise()
            cand = X
            if isinstance(X, _lib.Candidates):
                # a device batch lives in the normalised box: used as it is, under the condition MES states
                if not getattr(model, "normalize_input", False) or hasattr(model, "normalize"):
                    self._host_points(X)                                         # raises the TypeError
            else:
                cand = _lib.Candidates(model.gp.ctx, self._norm()(np.asarray(X, dtype=np.float64)))
            try:
                res = model.gp.kg(cand, self._rep_handle(), self._sn2(), self.include_self, want_values=want_values)
            finally:
                if cand is not X:
                    cand.close()
            vals, mx, am = res.values, res.max, res.argmax
        self.last_max, self.last_argmax = mx, int(am)
        return vals

    def compute(self, X, derivative=False, **kwargs):
        if derivative:
            raise NotImplementedError("KnowledgeGradient has no derivative")
        return self._evaluate(X, True)

    def argmax(self, X):
        """Index of the best candidate of X ((M, D) in the caller's input space, or a device batch ``_lib.Candidates`` in
        the normalised one): the fused call with only the maximiser coming back."""
        self._evaluate(X, False)
        return int(self.last_argmax)

    def argmax_sharded(self, comm, X_slice, global_offset):
        raise NotImplementedError("KnowledgeGradient has no candidate shard: multi-device and sharded forms are not "
                                  "implemented (use shard=False)")
