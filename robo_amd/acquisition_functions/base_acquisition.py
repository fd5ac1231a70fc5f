"""Acquisition plugin surface -- the contract of
robo/acquisition_functions/base_acquisition.py:4-69: ``__init__(model)``, ``update(model)``,
``compute(X, derivative=False, **kw)``, ``__call__ = compute``, ``get_json_data()``.

:class:`ClosedFormAcquisition` is the shared host shim of EI / LogEI / PI / LCB.  All
arithmetic runs on the device:

* model is a robo_amd GaussianProcess  -> fused path: cross-gram, triangular solve,
  variance/mean, acquisition and argmax in one C-ABI call (robo_acq_eval);
* any other BaseModel plugin            -> ``model.predict`` supplies (mean, var) and only the
  element-wise kernel runs (robo_acq_eval_moments).

The host plumbing every acquisition on ONE device shares is stated here once: ``staged_candidates`` (a host array becomes a
temporary device batch, a device batch is used as it is), ``host_points`` (a device batch back in the caller's input space,
and the one condition under which that is possible), ``refuse_multi_device``, ``predicted_moments`` and
:class:`OneDeviceAcquisition` (refusals, native / moments dispatch, ``compute`` / ``argmax``) -- what EHVI, ConstrainedEI and
the knowledge gradient derive from and MES and Thompson sampling borrow.
"""
import abc
import contextlib
import logging

import numpy as np

from robo_amd import _lib

logger = logging.getLogger(__name__)

MOMENT_ROWS = 512           # candidates per predict() call of the moments paths


class BaseAcquisitionFunction(object):
    __metaclass__ = abc.ABCMeta

    def __init__(self, model):
        self.model = model

    def update(self, model):
        """Called by the solver after the model was retrained."""
        self.model = model

    @abc.abstractmethod
    def compute(self, x, derivative=False):
        """Acquisition values at x (N, D) -> (N,)."""

    def __call__(self, x, **kwargs):
        return self.compute(x, **kwargs)

    def get_json_data(self):
        return {"type": __name__}

    def refine(self, X, n_starts=256, n_steps=50, step0=0.05):
        """Gradient-refined maximiser (device-resident multi-start ascent): EI / LogEI / PI / LCB over robo_amd GP models only."""
        raise TypeError("%s has no gradient refinement on the device: refine() is available for EI, LogEI, PI and LCB "
                        "over a robo_amd GaussianProcess (or MarginalizationGPMCMC over them)" % self.__class__.__name__)


    def select_batch(self, X, q, fantasy="kriging_believer", liar=None, diagnostics=False):
        """Greedy batch of q proposals with fantasised picks: EI / LogEI / PI / LCB over robo_amd GP models only."""
        raise TypeError("%s has no batch selection on the device: select_batch() is available for EI, LogEI, PI and LCB "
                        "over a robo_amd GaussianProcess (or MarginalizationGPMCMC over them)" % self.__class__.__name__)


def batch_liar(model, fantasy, liar):
    """the constant liar's value in the model's output scale: "min" | "mean" | "max" of the observed targets, or a float"""
    if fantasy != "constant_liar":
        return 0.0
    if liar is None:
        liar = "min"
    if isinstance(liar, str):
        if liar not in ("min", "mean", "max"):
            raise ValueError("liar must be 'min', 'mean', 'max' or a float, got %r" % (liar,))
        y = np.asarray(model.y, dtype=np.float64)
        v = float(getattr(np, liar)(y))
        if getattr(model, "normalize_output", False):
            v = v * model.y_std + model.y_mean
        return v
    return float(liar)


def joint_base_samples(acq, q, n_mc, z, rng):
    """the base samples of ``fantasy="joint"``: z (n_mc, q) as given, or drawn from ``rng``; TypeError for any acquisition
    other than EI (LogEI, PI and LCB have no joint form)"""
    from robo_amd.acquisition_functions.ei import EI
    if not isinstance(acq, EI):
        raise TypeError("fantasy='joint' (joint Monte-Carlo batch EI) is available for EI only (got %s)"
                        % type(acq).__name__)
    if z is not None:
        return np.ascontiguousarray(z, dtype=np.float64)
    if rng is None:
        rng = np.random.RandomState(np.random.randint(0, 2 ** 31 - 1))
    return rng.standard_normal((int(n_mc), max(int(q), 1)))


def batch_finish(acq, kind, model, res, cand):
    """shared tail of the select_batch() methods: the reference's EI guards act on pick 0's flags only (a floored variance
    at an already-picked point is expected, not a degenerate batch); the picked rows in the caller's input space"""
    acq.last_batch = res
    acq.last_max, acq.last_argmax = float(res.values[0]), int(res.indices[0])
    if kind == "ei":
        if res.flags[0] & _lib.FLAG_ZERO_SIGMA:       # ei.py:72-74: the batch collapses to [[0]], argmax 0
            res.indices[0] = 0
        elif res.flags[0] & _lib.FLAG_NEGATIVE_EI:
            raise ValueError
    pts = np.array([cand.point(int(i)) for i in res.indices[:res.n_made]]).reshape(res.n_made, cand.dim)
    lower, upper = np.asarray(model.lower, dtype=np.float64), np.asarray(model.upper, dtype=np.float64)
    return lower + (upper - lower) * pts


def refine_model_check(model, who, what="refine"):
    """the model requirements of the device refinement (and of the batch selection, what="select_batch"), as TypeError /
    NotImplementedError with a plain message"""
    # FabolasGP (models/fabolas_gp.py) is a GaussianProcess whose inputs go through its own normalize(): a basis function on
    # the fidelity column, so its input space is not the box [0, 1]^D the ascent is projected onto
    from robo_amd.models.fabolas_gp import FabolasGP
    if not (hasattr(model, "acquisition") and hasattr(model, "gp") and hasattr(model, "_normalised")) \
            or isinstance(model, FabolasGP):
        raise TypeError("%s.%s needs a robo_amd GaussianProcess model (got %s)" % (who, what, type(model).__name__))
    if not getattr(model, "normalize_input", False):
        raise TypeError("%s.%s works in the box [0, 1]^D of the normalised inputs: the model needs "
                        "normalize_input=True" % (who, what))
    if getattr(model, "devices", None):
        raise NotImplementedError("%s.%s runs on one device; multi-device sharding of it is not implemented"
                                  % (who, what))
    if not model.is_trained:
        raise Exception('Model has to be trained first!')


def refine_finish(acq, kind, model, res, cand):
    """shared tail of the refine() methods: the reference's EI guards on the sweep's flags, the point in the caller's
    input space"""
    acq.last_refine = res
    acq.last_max, acq.last_argmax = res.value, res.start_index
    x = res.x
    if kind == "ei":
        if res.flags & _lib.FLAG_ZERO_SIGMA:          # ei.py:72-74: the batch collapses to [[0]], argmax 0
            x = cand.point(0)
        elif res.flags & _lib.FLAG_NEGATIVE_EI:
            raise ValueError
    lower, upper = np.asarray(model.lower, dtype=np.float64), np.asarray(model.upper, dtype=np.float64)
    return lower + (upper - lower) * x


@contextlib.contextmanager
def staged_candidates(model, X):
    """The candidates of a fused call as a device batch: a ``_lib.Candidates`` is yielded as it is and left open; an array
    (caller's input space) goes through the model's own normalisation -- ``normalize`` where it has one (Fabolas), else the
    [0, 1] scaling -- into a temporary batch on the model's context, closed on exit."""
    if isinstance(X, _lib.Candidates):
        yield X
        return
    norm = model.normalize if hasattr(model, "normalize") else model._normalised
    cand = _lib.Candidates(model.gp.ctx, norm(np.asarray(X, dtype=np.float64)))
    try:
        yield cand
    finally:
        cand.close()


def refuse_foreign_batch(model, who, needs_box=False):
    """A device batch lives in the box [0, 1]^D of the model's normalised inputs.  It can be used as it is, or brought back
    to the caller's input space, only by a model that normalises its inputs with that scaling alone (``needs_box``: and
    says what the box is)."""
    if not getattr(model, "normalize_input", False) or hasattr(model, "normalize") \
            or (needs_box and (model.lower is None or model.upper is None)):
        raise TypeError("%s on a device candidate batch needs a model with normalize_input=True whose input space is the "
                        "normalised box (not a Fabolas model); pass the points as an array instead" % who)


def host_points(model, X, who, box=None):
    """An array as it is; a device batch in the caller's input space, under refuse_foreign_batch's condition.  ``box(model)``
    returns (lower, upper) or raises the caller's own error for a model without a box; without ``box`` a model without one
    is refused like the others."""
    if not isinstance(X, _lib.Candidates):
        return np.asarray(X, dtype=np.float64)
    refuse_foreign_batch(model, who, needs_box=box is None)
    lower, upper = box(model) if box is not None else (model.lower, model.upper)
    lower, upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    return lower + (upper - lower) * X.points()


def refuse_multi_device(models, who, why):
    """``devices=...`` models spread over several devices: NotImplementedError with the caller's reason ``why``"""
    for m in models:
        if getattr(m, "devices", None):
            raise NotImplementedError("%s runs on one device: %s (devices=%r)" % (who, why, m.devices))


def predicted_moments(models, X, rows=MOMENT_ROWS):
    """[(mean, var)] per model, flat fp64 (M,) each, from the models' predict() on ``rows`` candidates per call"""
    parts = [([], []) for _ in models]
    for r0 in range(0, X.shape[0], rows):
        for (mean, var), m in zip(parts, models):
            a, b = m.predict(X[r0:r0 + rows])[:2]
            mean.append(np.asarray(a, dtype=np.float64).ravel())
            var.append(np.asarray(b, dtype=np.float64).ravel())
    return [(np.concatenate(mean), np.concatenate(var)) for mean, var in parts]


def same_box_natives(models):
    """device GPs that take the same normalised candidates: one box, and one context after materialising -- what a fused
    call over several models needs (a Fabolas model is not counted).  Raises while one of them is not trained."""
    for m in models:
        if not (hasattr(m, "acquisition") and hasattr(m, "gp")) or hasattr(m, "normalize"):
            return False
    first = models[0]
    for m in models[1:]:
        if bool(m.normalize_input) != bool(first.normalize_input):
            return False
        if first.normalize_input and not (np.array_equal(first.lower, m.lower) and np.array_equal(first.upper, m.upper)):
            return False
    for m in models:
        if not m.is_trained:
            raise Exception('Model has to be trained first!')
        m._materialise()
    return all(m.gp.ctx is first.gp.ctx for m in models)


class OneDeviceAcquisition(BaseAcquisitionFunction):
    """An acquisition over one or more fitted models that runs on ONE device: native device models take a fused call on a
    device batch, every other model supplies its moments and the acquisition's own kernel alone runs on them.  A subclass
    supplies ``_models()`` (the first one's normalisation and context stage the candidates), ``_is_native()`` where its rule
    differs, ``_from_moments(Xhost, **how)`` and ``_fused(cand, want_values, **how)``, both -> (values or None, max, argmax);
    ``why_one_device`` is its reason for refusing ``devices=...`` models."""

    # no candidate shard (maximizers/random_sampling.py _check_candidate_shard)
    candidate_shard = False
    why_one_device = "multi-device and sharded forms are not implemented"

    def __init__(self, model):
        super(OneDeviceAcquisition, self).__init__(model)
        self.last_max = None
        self.last_argmax = None

    def _models(self):
        return [self.model]

    def _is_native(self):
        return hasattr(self.model, "acquisition") and hasattr(self.model, "gp")

    def _evaluate(self, X, want_values, **how):
        """-> (values or None, max, argmax); ``last_max`` / ``last_argmax`` are left to the caller"""
        who = self.__class__.__name__
        refuse_multi_device(self._models(), who, self.why_one_device)
        if isinstance(X, _lib.CandidateShards):
            raise NotImplementedError("%s runs on one device: candidate shards are not implemented" % who)
        first = self._models()[0]
        if not self._is_native():
            vals, mx, am = self._from_moments(self._host_points(X), **how)
        else:
            if not first.is_trained:
                raise Exception('Model has to be trained first!')
            first._materialise()
            if isinstance(X, _lib.Candidates):
                refuse_foreign_batch(first, who)
            with staged_candidates(first, X) as cand:
                vals, mx, am = self._fused(cand, want_values, **how)
        return vals, mx, int(am)

    def _host_points(self, X):
        return host_points(self._models()[0], X, self.__class__.__name__)

    def compute(self, X, derivative=False, **kwargs):
        if derivative:
            raise NotImplementedError("%s has no derivative" % self.__class__.__name__)
        vals, self.last_max, self.last_argmax = self._evaluate(X, True)
        return vals

    def argmax(self, X):
        """Index of the best candidate of X ((M, D) in the caller's input space, or a device batch ``_lib.Candidates`` in
        the normalised one): on the fused path only the maximiser comes back."""
        _, self.last_max, self.last_argmax = self._evaluate(X, False)
        return self.last_argmax

    def argmax_sharded(self, comm, X_slice, global_offset):
        raise NotImplementedError("%s has no candidate shard: multi-device and sharded forms are not implemented (use "
                                  "shard=False)" % self.__class__.__name__)


class ClosedFormAcquisition(BaseAcquisitionFunction):
    """EI / LogEI / PI / LCB on (mean, var, eta); subclasses set ``kind`` and the guards."""

    kind = None
    needs_eta = True

    def __init__(self, model, par=0.0, **kwargs):
        super(ClosedFormAcquisition, self).__init__(model)
        self.par = par
        self.last_max = None
        self.last_argmax = None

    def _is_native(self):
        return hasattr(self.model, "acquisition") and hasattr(self.model, "gp")

    def _eta(self, eta):
        if not self.needs_eta:
            return 0.0
        if eta is None:
            _, eta = self.model.get_incumbent()
        return float(eta)

    def _evaluate(self, X, eta):
        """-> (values (N,), flags)"""
        eta = self._eta(eta)
        if self._is_native():
            vals, mx, am, flags = self.model.acquisition(self.kind, self.par, eta, X)
        else:
            m, v = self.model.predict(X)
            vals, mx, am, flags = _lib.acq_from_moments(_lib.default_context(), self.kind, self.par, eta,
                                                        np.asarray(m, dtype=np.float64).ravel(),
                                                        np.asarray(v, dtype=np.float64).ravel())
        self.last_max, self.last_argmax = mx, am
        return vals, flags

    def argmax(self, X, eta=None):
        """Index of the best candidate without copying the values back (large-M maximisers)."""
        eta = self._eta(eta)
        if self._is_native():
            _, mx, am, flags = self.model.acquisition(self.kind, self.par, eta, X, want_values=False)
            self.last_max, self.last_argmax = mx, am
            if self.kind == "ei":
                # the reference's guards apply when maximising too (ei.py:72-74,86-88): any zero sigma
                # collapses the batch to [[0]] (argmax 0), any negative EI raises
                if flags & _lib.FLAG_ZERO_SIGMA:
                    return 0
                if flags & _lib.FLAG_NEGATIVE_EI:
                    raise ValueError
            return int(am)
        return int(np.argmax(self.compute(X, eta=eta)))

    def refine(self, X, n_starts=256, n_steps=50, step0=0.05, eta=None, diagnostics=False):
        """The maximiser refined by gradient ascent on the device (robo_acq_refine_cand): sweep over the candidates X
        ((M, D) in the caller's input space, or a device batch ``_lib.Candidates`` in the normalised one), the
        ``n_starts`` best of them climb ``n_steps`` projected steps in lock step -> the best point found, in the
        caller's input space.  ``last_refine`` keeps the library's result (value, start index, flags, diagnostics)."""
        model = self.model
        refine_model_check(model, self.__class__.__name__)
        model._materialise()
        with staged_candidates(model, X) as cand:       # (refine_model_check admits no model with a normalize() of its own)
            res = model.gp.refine(self.kind, self.par, self._eta(eta), cand, n_starts, n_steps, step0, diagnostics)
            return refine_finish(self, self.kind, model, res, cand)

    def select_batch(self, X, q, fantasy="kriging_believer", liar=None, diagnostics=False, eta=None, *, n_mc=128, z=None,
                     rng=None):
        """q proposals from ONE candidate batch X ((M, D) in the caller's input space, or a device batch
        ``_lib.Candidates`` in the normalised one) by greedy selection with fantasised picks (robo_acq_batch_cand): pick 0
        is the sweep's argmax; after every pick the posterior of all candidates is conditioned on a fantasy observation
        there -- the posterior mean (``kriging_believer``) or the constant ``liar`` ("min" | "mean" | "max" of the observed
        targets, or a float) -- with the hyper-parameters, the constant mean and the output normalisation frozen.
        -> (q', D) points in the caller's input space, q' < q only when a NaN winner ended the selection.  ``last_batch``
        keeps the library's result (indices, values, fantasies, flags, diagnostics).
        ``fantasy="joint"`` (EI only) picks by joint Monte-Carlo batch EI instead (robo_qei_batch_cand): no fantasies; the
        increments of q-EI over ``n_mc`` scenarios whose base samples are ``z`` (n_mc, q), or drawn from ``rng``;
        ``last_batch`` is then a ``_lib.QEIResult`` (gains, qei)."""
        model = self.model
        if fantasy == "joint":
            z = joint_base_samples(self, q, n_mc, z, rng)
        refine_model_check(model, self.__class__.__name__, "select_batch")
        model._materialise()
        with staged_candidates(model, X) as cand:
            if fantasy == "joint":
                res = model.gp.select_batch_joint(self.par, self._eta(eta), cand, q, z, diagnostics)
                return batch_finish(self, self.kind, model, res, cand)
            res = model.gp.select_batch(self.kind, self.par, self._eta(eta), cand, q, fantasy,
                                        batch_liar(model, fantasy, liar), diagnostics)
            return batch_finish(self, self.kind, model, res, cand)

    def argmax_sharded(self, comm, X_slice, global_offset):
        """Candidate shard (robo_amd.sharding.sharded_argmax): this rank's slice of the candidate matrix, whose first
        row has global index ``global_offset`` -> the GLOBAL np.argmax index, identical on every rank.  Posterior,
        acquisition, local argmax, the RCCL all-gather of the per-rank incumbents and the cross-rank tie-break are one
        library call (robo_acq_eval_cand_sharded); the reference's EI guards act on the flags OR-ed over all ranks,
        i.e. exactly as they would on the unsharded batch."""
        eta = self._eta(None)
        n_here = int(np.asarray(X_slice).shape[0])
        if not self._is_native():
            from robo_amd import sharding
            if n_here == 0:                           # more ranks than candidates: an empty shard still joins the exchange
                return sharding.allgather_argmax(-np.inf, -1)[1]
            vals = np.asarray(self.compute(X_slice), dtype=np.float64).reshape(-1)
            if vals.shape[0] != X_slice.shape[0]:
                vals = np.zeros(X_slice.shape[0])
            j = int(np.argmax(vals))
            return sharding.allgather_argmax(float(vals[j]), global_offset + j)[1]
        model = self.model
        if not model.is_trained:
            raise Exception('Model has to be trained first!')
        if n_here == 0:
            # an empty shard takes part in the SAME collective the other ranks issue inside robo_acq_eval_cand_sharded
            from robo_amd import sharding
            mx, am, flags = sharding.exchange_best(comm, lambda: None)
        else:
            model._materialise()
            norm = model.normalize if hasattr(model, "normalize") else model._normalised
            cand = _lib.Candidates(model.gp.ctx, norm(X_slice))
            try:
                _, mx, am, _, flags = comm.acq_sharded(model.gp, self.kind, self.par, eta, cand, global_offset)
            finally:
                cand.close()
        self.last_max, self.last_argmax = mx, am
        if self.kind == "ei":
            if flags & _lib.FLAG_ZERO_SIGMA:
                return 0
            if flags & _lib.FLAG_NEGATIVE_EI:
                raise ValueError
        return int(am)

    def _moment_gradients(self, X):
        """(mean, var, d mean / d x (M, D), d var / d x (M, D)) from ``model.predictive_gradients`` -- the
        protocol of ei.py:80-85 / pi.py:65-71 / lcb.py:66-68 (GPy shapes: dmdx (M, D, 1), dvdx (M, D))."""
        if not hasattr(self.model, "predictive_gradients"):
            raise NotImplementedError("%s: derivative=True needs model.predictive_gradients"
                                      % self.__class__.__name__)
        m, v = self.model.predict(X)
        dmdx, dvdx = self.model.predictive_gradients(X)
        dmdx = np.asarray(dmdx, dtype=np.float64)
        if dmdx.ndim == 3:
            dmdx = dmdx[:, :, 0]
        return np.asarray(m, dtype=np.float64), np.asarray(v, dtype=np.float64), dmdx, \
            np.asarray(dvdx, dtype=np.float64)
