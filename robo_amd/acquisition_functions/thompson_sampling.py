"""Thompson sampling by pathwise posterior samples (Matheron's rule; Wilson et al. 2020) -- no counterpart in the reference.

EI, PI, LCB, MES, KG and EHVI score a candidate from its posterior moments.  Thompson sampling draws a whole function from
the posterior and minimises it; q paths give q proposals from one call, without fantasies.  A path is

    f_s(x) = c + phi(x) . w_s + k(x, X) . alpha_s,     alpha_s = (K + noise I)^-1 (y - c - Phi_X w_s - sqrt(noise) eps_s)

with phi the random Fourier features of the prior (util/spectral.py) and w_s, eps_s standard normal.  The draws are made
here from ``rng``; all arithmetic runs on the device (robo_amd/csrc/paths.hip; the rule is stated in include/robo_hip.h).

* ``GaussianProcess``: all paths come from the one fitted GP.
* ``GaussianProcessMCMC``: every path first draws one hyper-parameter sample uniformly -- this is how Thompson sampling
  marginalises, so the class is NOT wrapped in ``MarginalizationGPMCMC``.  One paths object per distinct sample.

The acquisition value is -f_0(x) (path 0), so that the maximisers' argmax is the path's minimiser.  A path is a closed-form
differentiable function: ``refine`` / ``select_batch(refine=True)`` continue from the best candidates by projected gradient
descent on the paths themselves, all descents in one launch (robo_amd/csrc/paths_refine.hip), and ``value_and_gradient(X)``
returns a path's value and gradient from one evaluation.
"""
import numpy as np

from robo_amd import _lib
from robo_amd.acquisition_functions.base_acquisition import (BaseAcquisitionFunction, refine_model_check,
                                                             refuse_foreign_batch, refuse_multi_device, staged_candidates)
from robo_amd.util.spectral import draw_features


class ThompsonSampling(BaseAcquisitionFunction):

    # a path's minimiser over a slice of the candidates is not the batch's: no candidate shard
    # (maximizers/random_sampling.py _check_candidate_shard)
    candidate_shard = False

    def __init__(self, model, n_paths=1, n_features=1024, rng=None):
        super(ThompsonSampling, self).__init__(model)
        self.n_paths, self.n_features = int(n_paths), int(n_features)
        if not 1 <= self.n_paths <= _lib.PATHS_MAX:
            raise ValueError("n_paths = %d, must be in [1, %d]" % (self.n_paths, _lib.PATHS_MAX))
        if not 1 <= self.n_features <= _lib.PATHS_MAX_FEATURES:
            raise ValueError("n_features = %d, must be in [1, %d]" % (self.n_features, _lib.PATHS_MAX_FEATURES))
        self.rng = np.random.RandomState(np.random.randint(0, 10000)) if rng is None else rng
        self.last_max = None
        self.last_argmax = None
        self.hyper_index = None          # (n_paths,) the hyper-parameter sample behind every path (all 0 for a GaussianProcess)
        self._groups = []                # [(PosteriorPaths, path numbers it holds in order)]
        self._stale = True               # paths are drawn on the first use after update(): the model may not be trained yet

    # ---- the draws ----------------------------------------------------------------------------------------------------------
    def _sub_models(self):
        model = self.model
        subs = list(model.models) if hasattr(model, "models") else [model]
        refuse_multi_device([model] + subs, "ThompsonSampling", "multi-device models are not implemented")
        for m in subs:
            if not (hasattr(m, "acquisition") and hasattr(m, "gp") and hasattr(m, "_normalised")) or hasattr(m, "normalize"):
                raise TypeError("ThompsonSampling needs a robo_amd GaussianProcess or GaussianProcessMCMC model (got %s)"
                                % type(m).__name__)
        if not subs or not getattr(model, "is_trained", False):
            raise Exception('Model has to be trained first!')
        return subs

    def _close(self):
        for paths, _ in self._groups:
            paths.close()
        self._groups = []

    def update(self, model):
        """the retrained model: new features and new paths (drawn when first used)"""
        self.model = model
        self._stale = True

    def _draw(self, n_paths=None):
        """Per path, in path order: the hyper-parameter sample (``rng.randint(len(models))``, GaussianProcessMCMC only).
        Then per distinct sample in ascending order: (omega, phase) = draw_features, w = standard_normal((S_i, F)),
        eps = standard_normal((S_i, N))."""
        subs = self._sub_models()
        self._close()
        if n_paths is not None:
            self.n_paths = int(n_paths)
        S, F = self.n_paths, self.n_features
        if len(subs) > 1:
            self.hyper_index = np.array([int(self.rng.randint(len(subs))) for _ in range(S)], dtype=np.int64)
        else:
            self.hyper_index = np.zeros(S, dtype=np.int64)
        for i in sorted(set(self.hyper_index.tolist())):
            m = subs[i]
            m._materialise()
            members = np.flatnonzero(self.hyper_index == i)
            omega, phase = draw_features(m.kernel.kind, m.gp.dim, F, self.rng)
            w = self.rng.standard_normal((len(members), F))
            eps = self.rng.standard_normal((len(members), m.gp.n))
            self._groups.append((m.gp.sample_paths(omega, phase, w, eps), members))
        self._stale = False

    def _ready(self):
        if self._stale or not self._groups:
            self._draw()
        return self._sub_models()[0]

    # ---- evaluation ---------------------------------------------------------------------------------------------------------
    def _candidates(self, X, sub):
        """X as a device batch (staged_candidates; _sub_models admits no model with a normalize() of its own)"""
        if isinstance(X, _lib.CandidateShards):
            raise NotImplementedError("ThompsonSampling runs on one device: candidate shards are not implemented")
        if isinstance(X, _lib.Candidates):
            refuse_foreign_batch(sub, "ThompsonSampling")
        return staged_candidates(sub, X)

    def _evaluate(self, X, want_values, paths=None):
        """-> (values (S, m) or None, min (S,), argmin (S,)) in path order; ``paths``: only the groups that hold one of them"""
        sub = self._ready()
        with self._candidates(X, sub) as cand:
            S = self.n_paths
            vals = np.empty((S, cand.m)) if want_values else None
            mn, am = np.full(S, np.nan), np.full(S, -1, dtype=np.int64)
            for group, members in self._groups:
                if paths is not None and not np.intersect1d(members, paths).size:
                    continue
                r = group.evaluate(cand, want_values=want_values)
                mn[members], am[members] = r.min, r.argmin
                if want_values:
                    vals[members] = r.values
            return vals, mn, am

    def _group_of(self, path):
        """(PosteriorPaths, the path's number inside it) of the one group that holds ``path``"""
        for group, members in self._groups:
            at = np.flatnonzero(members == path)
            if at.size:
                return group, int(at[0])
        raise ValueError("path %d of %d" % (path, self.n_paths))

    def compute(self, X, derivative=False, **kwargs):
        """-f_0(X): the negated first path, (M,).  The gradient is ``value_and_gradient``'s second half."""
        if derivative:
            raise NotImplementedError("ThompsonSampling has no derivative in compute(): value_and_gradient(X) returns the "
                                      "value and the gradient of one consistent function")
        vals, mn, am = self._evaluate(X, True, paths=[0])
        self.last_max, self.last_argmax = -float(mn[0]), int(am[0])
        return -vals[0]

    def value_and_gradient(self, X):
        """(-f_0(X) (M,), -d f_0 / d X (M, D)) in the caller's input space (the chain rule through the input normalisation
        applied; a device batch ``_lib.Candidates``: in the normalised space), with the shapes the other acquisitions'
        ``derivative=True`` returns.  Both halves come from ONE evaluation of the descent kernel at X without steps
        (robo_paths_descend, slices of ``_lib.PATHS_MAX_DESCENTS`` points), so that a line search sees one consistent
        function.  That kernel forms the covariance entries from coordinate differences and the sweep forms them on the
        matrix pipe: these values may differ in the last bits from ``compute(X)``.  X must lie inside the model's box."""
        sub = self._ready()
        if isinstance(X, _lib.CandidateShards):
            raise NotImplementedError("ThompsonSampling runs on one device: candidate shards are not implemented")
        if isinstance(X, _lib.Candidates):
            refuse_foreign_batch(sub, "ThompsonSampling")
            Xn, chain = X.points(), 1.0
        else:
            Xn = np.ascontiguousarray(sub._normalised(np.asarray(X, dtype=np.float64)), dtype=np.float64)
            chain = 1.0
            if sub.normalize_input:       # x_normalised = (x - lower) / (upper - lower)
                chain = 1.0 / (np.asarray(sub.upper, dtype=np.float64) - np.asarray(sub.lower, dtype=np.float64))
        group, at = self._group_of(0)
        f, g = np.empty(Xn.shape[0]), np.empty(Xn.shape)
        for c in range(0, Xn.shape[0], _lib.PATHS_MAX_DESCENTS):
            part = Xn[c:c + _lib.PATHS_MAX_DESCENTS]
            r = group.descend(np.full(part.shape[0], at, dtype=np.int32), part, 0, 0.05)
            f[c:c + part.shape[0]], g[c:c + part.shape[0]] = r.value, r.grad
        return -f, -g * chain

    def refine(self, X, n_starts=256, n_steps=50, step0=0.05, diagnostics=False):
        """Path 0's minimiser refined by gradient descent on the path itself, on the device (robo_paths_refine_cand): the
        sweep over the candidates X ((M, D) in the caller's input space, or a device batch ``_lib.Candidates`` in the
        normalised one), the best rows of the ``n_starts`` best groups of 64 candidates descend ``n_steps`` projected steps
        in one launch -> the best point found, in the caller's input space.  ``last_refine`` keeps the library's result for
        the group that holds path 0 (its paths in the group's order), ``last_max`` is the negated value."""
        sub = self._ready()
        refine_model_check(sub, self.__class__.__name__)
        with self._candidates(X, sub) as cand:
            group, at = self._group_of(0)
            res = group.refine(cand, n_starts, n_steps, step0, diagnostics)
        self.last_refine = res
        self.last_max, self.last_argmax = -float(res.value[at]), int(res.start_index[at])
        lower, upper = np.asarray(sub.lower, dtype=np.float64), np.asarray(sub.upper, dtype=np.float64)
        return lower + (upper - lower) * res.x[at]

    def argmax(self, X):
        """Index of the first path's minimiser among X ((M, D) in the caller's input space, or a device batch
        ``_lib.Candidates`` in the normalised one): only the pick comes back."""
        _, mn, am = self._evaluate(X, False, paths=[0])
        self.last_max, self.last_argmax = -float(mn[0]), int(am[0])
        return int(am[0])

    def argmax_sharded(self, comm, X_slice, global_offset):
        raise NotImplementedError("ThompsonSampling has no candidate shard: multi-device and sharded forms are not "
                                  "implemented (use shard=False)")

    def select_batch(self, X, q, refine=False, n_starts=256, n_steps=50, step0=0.05, **unused):
        """q distinct rows of X, one per path -> (q, D) points in the caller's input space; ``last_batch`` keeps the row
        indices.  Path j takes its minimiser; when that row is taken already it takes its best row not yet taken (one
        read-back of that path's values).  With fewer than q paths, q paths are redrawn.  The fantasy arguments of the
        greedy selections are ignored: a path needs none.

        ``refine=True``: the q points are the q paths' minimisers refined on the device (``refine``'s rule, one fused call
        per group of paths); ``last_batch`` keeps the row every path's winning descent started from.  Different paths are
        different functions, so nothing is de-duplicated: equal points are kept."""
        q = int(q)
        sub = self._sub_models()[0]
        if refine:
            refine_model_check(sub, self.__class__.__name__, "select_batch")
        if self._stale or not self._groups or self.n_paths < q:
            self._draw(max(q, self.n_paths) if self.n_paths < q else None)
        with self._candidates(X, sub) as cand:
            if q < 1 or q > cand.m:
                raise ValueError("select_batch: q = %d outside 1 .. m = %d" % (q, cand.m))
            if refine:
                pts, rows, vals = np.empty((q, cand.dim)), np.empty(q, dtype=np.int64), np.empty(q)
                for group, members in self._groups:
                    keep = np.flatnonzero(members < q)
                    if keep.size:
                        r = group.refine(cand, n_starts, n_steps, step0)
                        pts[members[keep]], rows[members[keep]], vals[members[keep]] = r.x[keep], r.start_index[keep], r.value[keep]
                self.last_batch = rows
                self.last_max, self.last_argmax = -float(vals[0]), int(rows[0])
                lower, upper = np.asarray(sub.lower, dtype=np.float64), np.asarray(sub.upper, dtype=np.float64)
                return lower + (upper - lower) * pts
            _, mn, am = self._evaluate(cand, False, paths=np.arange(q))
            picks = []
            for j in range(q):
                i = int(am[j])
                if i in picks:
                    vals, _, _ = self._evaluate(cand, True, paths=[j])
                    neg = -vals[j]
                    neg[picks] = -np.inf                   # (NaN stays maximal among the rows not yet taken)
                    i = int(np.argmax(neg))
                picks.append(i)
            self.last_batch = np.array(picks, dtype=np.int64)
            self.last_max, self.last_argmax = -float(mn[0]), int(am[0])
            pts = np.array([cand.point(i) for i in picks]).reshape(q, cand.dim)
        if not sub.normalize_input:
            return pts
        lower, upper = np.asarray(sub.lower, dtype=np.float64), np.asarray(sub.upper, dtype=np.float64)
        return lower + (upper - lower) * pts

    def __deepcopy__(self, memo):
        import copy
        dup = ThompsonSampling.__new__(ThompsonSampling)
        memo[id(self)] = dup
        for k, v in self.__dict__.items():
            dup.__dict__[k] = [] if k == "_groups" else copy.deepcopy(v, memo)
        dup._stale = True
        return dup
