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
from robo_amd.acquisition_functions.base_acquisition import (MOMENT_ROWS, OneDeviceAcquisition, host_points,
                                                             refuse_multi_device)
from robo_amd.acquisition_functions.max_value_entropy_search import mes_box, mes_grid

# why a ``devices=...`` model is refused (refuse_multi_device)
KG_ONE_DEVICE = "multi-device and sharded forms of the knowledge gradient are not implemented"


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


class KnowledgeGradient(OneDeviceAcquisition):

    # (the discretisation is chosen over the whole box: no candidate shard)
    why_one_device = KG_ONE_DEVICE

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

    def _norm(self):
        return self.model.normalize if hasattr(self.model, "normalize") else self.model._normalised

    def discretisation_points(self):
        """this update's discretisation (nb, D) in the caller's input space (chosen on first use)"""
        if self._disc is None:
            refuse_multi_device([self.model], "KnowledgeGradient", KG_ONE_DEVICE)
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
        """(a model without a box: mes_box's ValueError)"""
        return host_points(self.model, X, "KnowledgeGradient", box=mes_box)

    def moments(self, X):
        """(s (M, nb) signed-as-given covariances with the discretisation, v (M,), mean (M,), disc_mean (nb,)) from the
        model's predict(full_cov=True), MOMENT_ROWS candidates per call"""
        Z = self.discretisation_points()
        nb = Z.shape[0]
        s, v, mean, disc = [], [], [], None
        for r0 in range(0, X.shape[0], MOMENT_ROWS):
            rows = X[r0:r0 + MOMENT_ROWS]
            mu, cov = self.model.predict(np.concatenate((rows, Z), axis=0), full_cov=True)
            mu, cov = np.asarray(mu, dtype=np.float64).ravel(), np.asarray(cov, dtype=np.float64)
            k = rows.shape[0]
            s.append(cov[:k, k:k + nb])
            v.append(np.diag(cov)[:k])
            mean.append(mu[:k])
            disc = mu[k:k + nb] if disc is None else disc
        return np.concatenate(s), np.concatenate(v), np.concatenate(mean), disc

    def _from_moments(self, Xhost):
        return _lib.kg_from_moments(_lib.default_context(), *self.moments(Xhost), sn2=self._sn2(),
                                    include_self=self.include_self)[:3]

    def _fused(self, cand, want_values):
        res = self.model.gp.kg(cand, self._rep_handle(), self._sn2(), self.include_self, want_values=want_values)
        return res.values, res.max, res.argmax
