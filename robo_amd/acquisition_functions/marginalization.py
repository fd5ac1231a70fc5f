"""Acquisition marginalised over GP hyper-parameter samples.

Semantics of robo/acquisition_functions/marginalization.py:11-121: one estimator (a deep
copy of the wrapped acquisition function) per ``model.models[i]``; ``update`` re-points each
estimator at the retrained sub-model; ``compute`` returns the mean over samples, accumulated
in sample order (NumPy's axis-0 mean).

When every sub-model is a device-resident robo_amd GaussianProcess and the wrapped function
is EI/LogEI/PI/LCB, the S posteriors, S acquisition vectors, their ordered sum and the final
argmax are produced by ONE C-ABI call on a shared candidate upload
(robo_acq_eval_marginal_cand); otherwise the estimators are evaluated one by one exactly
like the reference does.
"""
import logging
from copy import deepcopy

import numpy as np

from robo_amd import _lib
from robo_amd.acquisition_functions.base_acquisition import (BaseAcquisitionFunction, ClosedFormAcquisition,
                                                             refuse_multi_device, staged_candidates)

logger = logging.getLogger(__name__)


def _ig_update_from_points():
    from robo_amd.acquisition_functions.information_gain import InformationGain
    return InformationGain._update_from_points


class MarginalizationGPMCMC(BaseAcquisitionFunction):

    def __init__(self, acquisition_func):
        self.acquisition_func = acquisition_func
        self.model = acquisition_func.model
        self.cost_model = getattr(acquisition_func, "cost_model", None)
        self.estimators = []
        self._build_estimators()
        self.last_max = None
        self.last_argmax = None
        # sample shard (SURVEY.md 8e axis 2): with one process per GPU and ``sample_shard = True`` every rank
        # evaluates only ITS hyper-parameter samples on all candidates; the per-rank partial sums are exchanged
        # and added in rank order (robo_amd.sharding.allgather_ordered_sum)
        self.sample_shard = False
        self._kg_rep = None         # knowledge gradient: the shared discretisation as a device handle, per update()

    def _build_estimators(self):
        for i in range(len(self.model.models)):
            # detach the (possibly device-resident) model while copying: the copy gets its own
            # sub-model right below, as in marginalization.py:36-40
            model, self.acquisition_func.model = self.acquisition_func.model, None
            try:
                estimator = deepcopy(self.acquisition_func)
            finally:
                self.acquisition_func.model = model
            estimator.model = self.model.models[i]
            if self.cost_model is not None and len(self.cost_model.models) > 0:
                estimator.cost_model = self.cost_model.models[i]
            self.estimators.append(estimator)

    def update(self, model, cost_model=None, **kwargs):
        self.model = model
        self._kg_drop()
        if cost_model is not None:
            self.cost_model = cost_model
        if len(self.estimators) != len(self.model.models):
            self.estimators = []
            self._build_estimators()
        if cost_model is None and not kwargs and self._update_representers_batched():
            return
        for i in range(len(self.model.models)):
            if cost_model is not None:
                self.estimators[i].update(self.model.models[i], self.cost_model.models[i], **kwargs)
            else:
                self.estimators[i].update(self.model.models[i], **kwargs)

    # ---- entropy search: the representer chains of all hyper-parameter samples in one call per context ------------------------
    def _representer_plan(self):
        """the estimators' chain inputs (InformationGain._chain_inputs) grouped by their sub-model's context, in sample order
        -> [(indices, inputs)], or None where update() stays one estimator after the other"""
        from robo_amd.acquisition_functions.information_gain import InformationGain
        est = self.estimators
        if not est or not all(isinstance(e, InformationGain) and e._representers() == "device" for e in est):
            return None
        inputs = []
        for e, m in zip(est, self.model.models):
            e.model = m
            e.sampling_acquisition.update(m)
            inputs.append(e._chain_inputs())           # (Fabolas sub-models raise NotImplementedError here)
        if any(x is None for x in inputs):
            return None
        e0, x0 = est[0], inputs[0]
        for e, x in zip(est, inputs):
            if x[1:3] != x0[1:3] or x[4] != x0[4] or (e.Nb, e.D, e.sampler_steps) != (e0.Nb, e0.D, e0.sampler_steps) \
                    or not (np.array_equal(e.lower, e0.lower) and np.array_equal(e.upper, e0.upper)):
                return None
        groups = {}
        for i, x in enumerate(inputs):
            groups.setdefault(id(x[0].ctx), []).append(i)
        for idx in groups.values():
            if len({inputs[i][0].n for i in idx}) != 1 or len({id(inputs[i][0]) for i in idx}) != len(idx):
                return None
        return [(idx, [inputs[i] for i in idx]) for idx in groups.values()]

    def _update_representers_batched(self):
        """update() of entropy-search estimators with ``representers="device"`` over trained device GPs: every estimator's
        restarts and draws in estimator order, ONE robo_rep_sample_batch per context, a retry (up to 5 attempts, as
        InformationGain.sample_representer_points) only for the chains that hit -inf, then the rest of each estimator's
        update from its points -- with ``ep="device"`` the EP of all beliefs of a context in one joint_min_batch.
        -> False: nothing was done, update() goes estimator by estimator"""
        from robo_amd.acquisition_functions.information_gain import chain_record
        from robo_amd.util import epmgp
        plan = self._representer_plan()
        if plan is None:
            return False
        est = self.estimators
        e0 = est[0]
        T, half = e0.sampler_steps, e0.Nb // 2
        for e in est:
            if hasattr(e, "_single_device"):
                e._single_device()
            e.sn2 = e.model.get_noise()
        pending = list(range(len(est)))
        alone = []                                           # estimators whose chain has to run the host's way
        for _ in range(5):
            if not pending:
                break
            start, draws = {}, {}
            for i in pending:                                # estimator order: restarts, then the sampler's stream
                e = est[i]
                start[i] = e.lower + (e.upper - e.lower) * e.rng.uniform(size=(e.Nb, e.D))
                draws[i] = _lib.mcmc_draws(e._sampler_stream(), T, half)
            for idx, inputs in plan:
                sel = [(i, x) for i, x in zip(idx, inputs) if i in start]
                if not sel:
                    continue
                ids, xs = [i for i, _ in sel], [x for _, x in sel]
                kind, par, normalize = xs[0][1], xs[0][2], xs[0][4]
                pos0 = np.array([start[i] for i in ids])
                uz, pa, ua = (np.array([draws[i][j] for i in ids]) for j in range(3))
                try:
                    pos, lnp, acc, flags, _ = _lib.rep_sample_batch([x[0] for x in xs], kind, par, [x[3] for x in xs],
                                                                    e0.lower, e0.upper, normalize, pos0, None, T, uz, pa, ua)
                except _lib.RoboBadShape:
                    if len(pending) == len(est):
                        return False                         # half an ensemble does not fit the solve workspace
                    raise
                for j, i in enumerate(ids):
                    if flags[j] & _lib.FLAG_NAN:
                        raise ValueError("lnprob returned NaN.")
                    if kind == "ei" and flags[j] & (_lib.FLAG_ZERO_SIGMA | _lib.FLAG_NEGATIVE_EI):
                        alone.append(i)                      # EI's per-batch guards: that estimator's own host loop
                        continue
                    est[i].zb, est[i].lmb = pos[j], lnp[j]
            pending = [i for i in pending if i not in alone and np.any(np.isinf(est[i].lmb))]
        for i in alone:
            saved, est[i].representers = est[i].representers, "host"
            try:
                est[i].sample_representer_points()
            finally:
                est[i].representers = saved
        for e in est:
            e._shape_representers()
        for idx, inputs in plan:
            group = [est[i] for i in idx]
            batched_ep = type(group[0])._update_from_points is _ig_update_from_points() and \
                all((e.ep or epmgp.default_backend) == "device" for e in group)
            if not batched_ep:
                for e in group:
                    e._update_from_points()
                continue
            beliefs = [e._belief() for e in group]
            res = epmgp.joint_min_batch(np.array([b[0] for b in beliefs]), np.array([b[1] for b in beliefs]), True,
                                        ctx=inputs[0][0].ctx)
            for j, e in enumerate(group):
                e._update_from_points(ep=tuple(r[j] for r in res))
        return True

    def _device_groups(self):
        """Single-process multi-GPU (``GaussianProcessMCMC(devices=...)``): the estimators grouped by the device slot
        their sub-model lives on, or None when this is not such a model / not a fused closed-form case."""
        devices = getattr(self.model, "devices", None)
        if not devices or self._shard() is not None or not self.estimators:
            return None
        if not isinstance(self.acquisition_func, ClosedFormAcquisition):
            return None
        multi = _lib.multi_for(devices)
        groups = [[] for _ in multi.ctxs]
        for e in self.estimators:
            gp = getattr(e.model, "gp", None)
            if not isinstance(gp, _lib.DeviceGP) or not getattr(e.model, "is_trained", False):
                return None
            slot = next((g for g, c in enumerate(multi.ctxs) if c is gp.ctx), None)
            if slot is None or (groups[slot + 1:] and any(groups[slot + 1:])):
                return None                          # not on the list, or not in contiguous sample order
            groups[slot].append(e)
        return multi, groups

    def _multi_eval(self, X_test, want_values):
        """sample shard over the devices of ONE process (robo_acq_eval_marginal_cand_multi): every device accumulates its
        samples' acquisition values on all candidates; the partial sums are added in device order on the first device"""
        multi, groups = self._device_groups()
        if isinstance(X_test, _lib.Candidates):
            X_test = self._host_points(X_test)       # every device needs the whole batch: through the host, once
        m0 = self.estimators[0].model
        Xn = (m0.normalize if hasattr(m0, "normalize") else m0._normalised)(X_test)
        cands = [_lib.Candidates(c, Xn) if (groups[g] or g == 0) else None for g, c in enumerate(multi.ctxs)]
        ref = self.estimators[0]
        try:
            vals, mx, am, flags = multi.acq_marginal([[e.model.gp for e in grp] for grp in groups], ref.kind, ref.par,
                                                     [[e._eta(None) for e in grp] for grp in groups], cands, want_values)
        finally:
            for c in cands:
                if c is not None:
                    c.close()
        self.last_max, self.last_argmax = mx, am
        return vals, flags

    def _native(self):
        if self._shard() is not None:
            return False
        if not isinstance(self.acquisition_func, ClosedFormAcquisition) or not self.estimators:
            return False
        gps = [getattr(e.model, "gp", None) for e in self.estimators]
        return all(isinstance(g, _lib.DeviceGP) for g in gps) and len({id(g.ctx) for g in gps}) == 1 \
            and all(getattr(e.model, "is_trained", False) for e in self.estimators)

    def _shard(self):
        # the opt-in flag FIRST: dist_info() is collective on first use (the communicator id is broadcast, every rank
        # joins ncclCommInitRank) and must not run because a torch process group merely exists
        if not self.sample_shard:
            return None
        from robo_amd import sharding
        _, rank, world = sharding.dist_info()
        if world == 1:
            return None
        return sharding.shard_range(len(self.estimators), rank, world)

    def _sharded_eval(self, X_test):
        """mean over ALL samples from per-rank partial sums; -> values (M,), identical on every rank"""
        from robo_amd import sharding
        b, e = self._shard()
        est = self.estimators[b:e]
        S = len(self.estimators)
        if isinstance(X_test, _lib.Candidates):
            # a device-generated batch lives in the normalised space of ITS maximiser's model; the sample shard
            # evaluates host coordinates (every rank must see the same points): bring them back once
            X_test = self._host_points(X_test)
        comm = sharding.comm()
        # which exchange runs must not depend on the rank: decided from the CLASSES of all estimators' models
        fused = isinstance(self.acquisition_func, ClosedFormAcquisition) and \
            all(hasattr(x.model, "acquisition") and hasattr(x.model, "gp") for x in self.estimators)
        if fused:
            # partial sums on the device, all-gathered and added in rank order inside the library
            # (robo_acq_eval_marginal_cand_sharded); a rank without samples (S < world) takes part with an empty sum
            for x in est:
                if not x.model.is_trained:
                    raise Exception('Model has to be trained first!')
                x.model._materialise()
            ref = est[0] if est else self.estimators[0]
            if est:
                m0 = ref.model
                Xn = (m0.normalize if hasattr(m0, "normalize") else m0._normalised)(X_test)
            else:
                Xn = np.zeros_like(np.asarray(X_test, dtype=np.float64))      # never evaluated: no local sample
            cand = _lib.Candidates(comm.ctx, Xn)
            try:
                vals, mx, am, flags = comm.acq_marginal_sharded([x.model.gp for x in est], S, ref.kind, ref.par,
                                                                [x._eta(None) for x in est], cand)
            finally:
                cand.close()
            self.last_max, self.last_argmax = mx, am
            if ref.kind == "ei" and flags & _lib.FLAG_NEGATIVE_EI:
                raise ValueError                      # the flags are OR-ed over all ranks: every rank raises
            return vals
        part = np.zeros(X_test.shape[0])
        for x in est:
            part = part + np.asarray(x.compute(X_test), dtype=np.float64).reshape(-1)
        return sharding.allgather_ordered_sum(part) / S

    def _host_points(self, cand):
        """coordinates of a device candidate batch in the caller's input space"""
        m0 = self.estimators[0].model
        P = cand.points()
        lower, upper = np.asarray(m0.lower, dtype=np.float64), np.asarray(m0.upper, dtype=np.float64)
        if hasattr(m0, "normalize") and not getattr(m0, "normalize_input", False):
            raise TypeError("device-generated candidates are not supported with Fabolas sub-models")
        return lower + (upper - lower) * P

    def _native_eval(self, X_test, want_values):
        est = self.estimators
        models = [e.model for e in est]
        gps = [m.gp for m in models]
        # every estimator asks its own sub-model for the incumbent (marginalization.py:40, ei.py:68)
        eta = np.array([e._eta(None) for e in est])
        # FabolasGP sub-models map their inputs through normalize() ([0,1] scaling of the configuration
        # columns + basis function on the fidelity column, fabolas_gp.py:122-126); plain GPs through the
        # [0,1] normalisation
        with staged_candidates(models[0], X_test) as cand:
            vals, mx, am, flags = _lib.acq_marginal(gps, est[0].kind, est[0].par, eta, cand, want_values)
        self.last_max, self.last_argmax = mx, am
        return vals, flags

    # ---- max-value entropy search: every hyper-parameter sample has its own sampled minima y*_s -----------------------------
    def _is_mes(self):
        from robo_amd.acquisition_functions.max_value_entropy_search import MES
        return isinstance(self.acquisition_func, MES)

    def _mes_native(self):
        """all sub-models are trained device GPs on one context -> the marginal entry points (robo_mes_eval_marginal_cand)"""
        from robo_amd.acquisition_functions.max_value_entropy_search import MES_ONE_DEVICE
        refuse_multi_device([self.model], "MarginalizationGPMCMC(MES)", MES_ONE_DEVICE)
        if self.sample_shard:
            raise NotImplementedError("MarginalizationGPMCMC(MES) has no sample shard: y* is sampled per hyper-parameter "
                                      "sample on one device")
        if not self.estimators:
            return False
        for e in self.estimators:
            refuse_multi_device([e.model], "MarginalizationGPMCMC(MES)", MES_ONE_DEVICE)
            if not (hasattr(e.model, "acquisition") and hasattr(e.model, "gp")) or hasattr(e.model, "normalize") \
                    or not getattr(e.model, "is_trained", False):
                return False
            e.model._materialise()
        gps = [e.model.gp for e in self.estimators]
        return all(isinstance(g, _lib.DeviceGP) for g in gps) and len({id(g.ctx) for g in gps}) == 1

    def _mes_marginal(self, X, want_values, diagnostics=False):
        """the fused marginal call with X as every sample's discretisation; fresh uniforms (S, K) from the wrapped
        function's rng"""
        from robo_amd.acquisition_functions.max_value_entropy_search import mes_uniforms
        f, est = self.acquisition_func, self.estimators
        gps = [e.model.gp for e in est]
        etas = np.array([e._eta() for e in est])
        with staged_candidates(est[0].model, X) as cand:      # (_mes_native admits no model with a normalize() of its own)
            u = mes_uniforms(f.rng, (len(est), f.n_samples))
            return _lib.mes_marginal(gps, etas, cand, u, f.clamp, want_values, diagnostics)

    def _mes_compute(self, X_test):
        """the paper's form: per model update one set of y*_s per sample, drawn over ONE discretisation by the fused
        marginal call; then the element-wise half at X per sample, averaged in sample order"""
        from robo_amd.acquisition_functions.max_value_entropy_search import mes_grid
        f, est = self.acquisition_func, self.estimators
        if isinstance(X_test, _lib.Candidates):
            X_test = self._host_points(X_test)
        if any(e._ystar is None for e in est):
            ystar = self._mes_marginal(mes_grid(est[0].model, f.rng, f.n_grid), False).ystar
            for s, e in enumerate(est):
                e._ystar = ystar[s]
        total = np.zeros(np.asarray(X_test).shape[0])
        for e in est:
            m, v = e.model.gp.predict(e.model._normalised(np.asarray(X_test, dtype=np.float64)))
            total = total + _lib.mes_from_moments(e.model.gp.ctx, m, v, e._ystar)[0]
        vals = total / len(est)
        self.last_max, self.last_argmax = float(np.max(vals)), int(np.argmax(vals))
        self.last_ystar = np.array([e._ystar for e in est])
        return vals

    # ---- knowledge gradient: one discretisation for all hyper-parameter samples, re-solved per sample ------------------------
    def _is_kg(self):
        from robo_amd.acquisition_functions.knowledge_gradient import KnowledgeGradient
        return isinstance(self.acquisition_func, KnowledgeGradient)

    def _kg_drop(self):
        if getattr(self, "_kg_rep", None) is not None:
            self._kg_rep.close()
        self._kg_rep = None

    def _kg_native(self):
        """all sub-models are trained device GPs on one context -> the marginal entry point (robo_kg_eval_marginal_cand)"""
        from robo_amd.acquisition_functions.knowledge_gradient import KG_ONE_DEVICE
        refuse_multi_device([self.model], "MarginalizationGPMCMC(KnowledgeGradient)", KG_ONE_DEVICE)
        if self.sample_shard:
            raise NotImplementedError("MarginalizationGPMCMC(KnowledgeGradient) has no sample shard: multi-device and "
                                      "sharded forms of the knowledge gradient are not implemented")
        if not self.estimators:
            return False
        for e in self.estimators:
            refuse_multi_device([e.model], "MarginalizationGPMCMC(KnowledgeGradient)", KG_ONE_DEVICE)
            if not (hasattr(e.model, "acquisition") and hasattr(e.model, "gp")) or hasattr(e.model, "normalize") \
                    or not getattr(e.model, "is_trained", False):
                return False
            e.model._materialise()
        gps = [e.model.gp for e in self.estimators]
        return all(isinstance(g, _lib.DeviceGP) for g in gps) and len({id(g.ctx) for g in gps}) == 1

    def _kg_marginal(self, X, want_values, diagnostics=False):
        """the fused marginal call; the discretisation comes from the first sample's model (as _mes_compute takes its
        grid) and is shared by every estimator for this update()"""
        from robo_amd.acquisition_functions.knowledge_gradient import kg_discretisation
        f, est = self.acquisition_func, self.estimators
        gps = [e.model.gp for e in est]
        if self._kg_rep is None:
            Z = est[0]._disc
            if Z is None:
                Z = kg_discretisation(est[0].model, f.rng, f.n_disc, f.n_grid, f.discretisation)
            for e in est:
                e._disc = Z
                e._drop_rep()
            self._kg_rep = _lib.Candidates(gps[0].ctx, est[0].model._normalised(Z))
        sn2s = np.array([e._sn2() for e in est])
        with staged_candidates(est[0].model, X) as cand:      # (_kg_native admits no model with a normalize() of its own)
            res = _lib.kg_marginal(gps, cand, self._kg_rep, sn2s, f.include_self, want_values, diagnostics)
        self.last_max, self.last_argmax = res.max, res.argmax
        return res

    def compute(self, X_test, derivative=False):
        if self._is_kg():
            if derivative:
                raise NotImplementedError("KnowledgeGradient has no derivative")
            if self._kg_native():
                if isinstance(X_test, _lib.Candidates):
                    self.estimators[0]._host_points(X_test)        # the condition a device batch comes under
                return self._kg_marginal(X_test, True).values
        if self._is_mes():
            if derivative:
                raise NotImplementedError("MES has no derivative")
            if self._mes_native():
                return self._mes_compute(X_test)
        if not derivative and self._shard() is not None:
            return self._sharded_eval(X_test)
        fused = None
        if not derivative and self._device_groups() is not None:
            fused = self._multi_eval
        elif not derivative and self._native():
            fused = self._native_eval
        if fused is not None:
            vals, flags = fused(X_test, True)
            if self.estimators[0].kind == "ei":
                if flags & _lib.FLAG_ZERO_SIGMA:
                    # some estimator would have returned [[0]] (ei.py:72-74); keep the reference's
                    # per-estimator behaviour by falling through to the one-by-one evaluation
                    pass
                elif flags & _lib.FLAG_NEGATIVE_EI:
                    raise ValueError
                else:
                    return vals
            else:
                return vals
        if isinstance(X_test, _lib.Candidates):
            X_test = self._host_points(X_test)       # host loop below: the reference's per-estimator evaluation
        acquisition_values = np.zeros([len(self.model.models), X_test.shape[0]])
        by_ctx = {}
        for i, e in enumerate(self.estimators):
            # every context an estimator drives: its model's and, for the per-unit-cost form, its cost model's -- a context
            # (stream, pinned read-back, scratch) is not thread-safe, so it may belong to ONE thread only
            key = []
            for mdl in (getattr(e, "model", None), getattr(e, "cost_model", None)):
                gp = getattr(mdl, "gp", None)
                if mdl is not None:
                    key.append(id(gp.ctx) if isinstance(gp, _lib.DeviceGP) else None)
            by_ctx.setdefault(tuple(key), []).append(i)
        seen = [c for key in by_ctx for c in set(key)]
        disjoint = len(seen) == len(set(seen)) and None not in seen
        if len(by_ctx) > 1 and disjoint and getattr(self.model, "devices", None):
            # sub-models on several devices of this process (any acquisition function, e.g. the information gain per unit
            # cost of Fabolas): one host thread per device walks its estimators -- the library calls release the GIL, so
            # the devices work at the same time; the mean is still taken in sample order
            from concurrent.futures import ThreadPoolExecutor

            def run(idx):
                for i in idx:
                    acquisition_values[i] = self.estimators[i].compute(X_test, derivative=derivative)
            with ThreadPoolExecutor(max_workers=len(by_ctx)) as pool:
                for f in [pool.submit(run, idx) for idx in by_ctx.values()]:
                    f.result()
            return acquisition_values.mean(axis=0)
        for i in range(len(self.model.models)):
            acquisition_values[i] = self.estimators[i].compute(X_test, derivative=derivative)
        return acquisition_values.mean(axis=0)

    def refine(self, X_test, n_starts=256, n_steps=50, step0=0.05, diagnostics=False):
        """Gradient-refined maximiser of the marginalised acquisition (robo_acq_refine_marginal_cand): as
        ClosedFormAcquisition.refine, value and gradient averaged over the hyper-parameter samples in sample order."""
        from robo_amd.acquisition_functions.base_acquisition import refine_finish, refine_model_check
        if not isinstance(self.acquisition_func, ClosedFormAcquisition) or not self.estimators:
            raise TypeError("MarginalizationGPMCMC.refine is available for EI, LogEI, PI and LCB only (got %s)"
                            % type(self.acquisition_func).__name__)
        if getattr(self.model, "devices", None) or self._shard() is not None:
            raise NotImplementedError("MarginalizationGPMCMC.refine runs on one device; multi-device and multi-process "
                                      "sharding of the refinement is not implemented")
        for e in self.estimators:
            refine_model_check(e.model, "MarginalizationGPMCMC")
            e.model._materialise()
        est = self.estimators
        gps = [e.model.gp for e in est]
        if len({id(g.ctx) for g in gps}) != 1:
            raise NotImplementedError("MarginalizationGPMCMC.refine: the sub-models live on several contexts")
        eta = np.array([e._eta(None) for e in est])
        m0 = est[0].model
        with staged_candidates(m0, X_test) as cand:
            res = _lib.acq_refine(gps, est[0].kind, est[0].par, eta, cand, n_starts, n_steps, step0, diagnostics)
            return refine_finish(self, est[0].kind, m0, res, cand)

    def select_batch(self, X_test, q, fantasy="kriging_believer", liar=None, diagnostics=False, *, n_mc=128, z=None,
                     rng=None):
        """Greedy batch of q proposals under the marginalised acquisition (robo_acq_batch_marginal_cand): as
        ClosedFormAcquisition.select_batch; every hyper-parameter sample is conditioned on its own fantasy (its own posterior
        mean for the kriging believer) and keeps its own incumbent, the values are averaged in sample order.
        ``fantasy="joint"`` (EI only): joint Monte-Carlo batch EI (robo_qei_batch_marginal_cand), the base samples shared
        by the hyper-parameter samples."""
        from robo_amd.acquisition_functions.base_acquisition import (batch_finish, batch_liar, joint_base_samples,
                                                                     refine_model_check)
        if fantasy == "joint":
            z = joint_base_samples(self.acquisition_func, q, n_mc, z, rng)
        if not isinstance(self.acquisition_func, ClosedFormAcquisition) or not self.estimators:
            raise TypeError("MarginalizationGPMCMC.select_batch is available for EI, LogEI, PI and LCB only (got %s)"
                            % type(self.acquisition_func).__name__)
        if getattr(self.model, "devices", None) or self._shard() is not None:
            raise NotImplementedError("MarginalizationGPMCMC.select_batch runs on one device; multi-device and "
                                      "multi-process sharding of the batch selection is not implemented")
        for e in self.estimators:
            refine_model_check(e.model, "MarginalizationGPMCMC", "select_batch")
            e.model._materialise()
        est = self.estimators
        gps = [e.model.gp for e in est]
        if len({id(g.ctx) for g in gps}) != 1:
            raise NotImplementedError("MarginalizationGPMCMC.select_batch: the sub-models live on several contexts")
        eta = np.array([e._eta(None) for e in est])
        m0 = est[0].model
        with staged_candidates(m0, X_test) as cand:
            if fantasy == "joint":
                res = _lib.qei_batch(gps, est[0].par, eta, cand, q, z, diagnostics)
                return batch_finish(self, est[0].kind, m0, res, cand)
            res = _lib.acq_batch(gps, est[0].kind, est[0].par, eta, cand, q, fantasy, batch_liar(m0, fantasy, liar),
                                 diagnostics)
            return batch_finish(self, est[0].kind, m0, res, cand)

    def argmax(self, X_test):
        if self._is_kg() and self._kg_native():
            return int(self._kg_marginal(X_test, False).argmax)
        if self._is_mes() and self._mes_native():
            res = self._mes_marginal(X_test, False)
            self.last_max, self.last_argmax, self.last_ystar = res.max, res.argmax, res.ystar
            return int(res.argmax)
        if self._shard() is not None:
            return int(np.argmax(self._sharded_eval(X_test)))
        fused = self._multi_eval if self._device_groups() is not None else (self._native_eval if self._native() else None)
        if fused is not None:
            _, flags = fused(X_test, False)
            if self.estimators[0].kind != "ei" or not flags & (_lib.FLAG_ZERO_SIGMA | _lib.FLAG_NEGATIVE_EI):
                return int(self.last_argmax)
            # an estimator would have collapsed to [[0]] / raised (ei.py:72-74,86-88): same path as compute()
        return int(np.argmax(self.compute(X_test)))
