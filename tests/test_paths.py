"""Pathwise posterior samples and Thompson sampling (robo_amd/csrc/paths.hip, api_paths.hip: robo_paths_create,
robo_paths_eval_cand, robo_paths_destroy; util/spectral.py, _lib.PosteriorPaths, the ThompsonSampling class and
bayesian_optimization(acquisition_func="thompson")) against tests/paths_oracle.py.

CPU: through the interpreter (tests/hipemu).  -m gpu: the same checks at the same small shapes on the MI355X, plus the fused
case at N = 256, D = 4, F = 1024, S = 8, m = 32 773.

The oracle is the rule of include/robo_hip.h in np.longdouble, fed THE DEVICE'S OWN DOUBLES (scaled rows as cov_oracle.scale
makes them; the same omega, phase, w, eps).  The value bound is cov_checks.check_feeds's form, per case and path:

    |f_dev - f_orc| <= MU_RTOL |f_orc| + MU_ATOL max(1, max |f_orc|) + 20 dev

with dev the largest deviation of the same routine in np.float64 from the long-double oracle over the case's candidates (the
problem's own conditioning: alpha grows like sqrt(N / noise)), MU_* from tests/_tol.py.  Largest observed error / bound:
    interpreter:   0.095 (value cases), 0.0005 (class replay)
    MI355X:        0.111 (value cases), 0.0005 (class replay), 0.0008 (fused large)
Before robo_paths_create refined alpha by one step against K the case ('matern52', N = 63, D = 1, noise 1e-6, output
normalisation) stood at 1.21 of the bound on the MI355X (0.326 under the interpreter); it is at 0.061 (0.063) now
(NOTES.md "Pathwise posterior samples").
"""
import os
import sys

import numpy as np
import pytest

from robo_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import cov_oracle as CO  # noqa: E402
import paths_oracle as PO  # noqa: E402
from _tol import MU_ATOL, MU_RTOL  # noqa: E402
from robo_amd.util.spectral import draw_features  # noqa: E402

AMP = 1.3
# (kind, N, D, F, S, m, noise, output normalisation): every listed size of every axis, both kinds, both noises
CASES = [
    ("matern52", 1, 1, 1, 1, 1, 1e-2, False),
    ("rbf", 63, 3, 63, 2, 127, 1e-6, True),
    ("matern52", 64, 16, 64, 15, 128, 1e-2, True),
    ("rbf", 65, 17, 65, 16, 129, 1e-2, False),
    ("matern52", 130, 3, 300, 17, 401, 1e-6, False),
    ("rbf", 257, 16, 300, 64, 401, 1e-6, True),
    ("matern52", 257, 17, 1, 64, 1, 1e-2, True),
    ("rbf", 1, 3, 300, 17, 127, 1e-6, False),
    ("matern52", 63, 1, 64, 16, 129, 1e-6, True),
    ("rbf", 64, 1, 63, 1, 128, 1e-2, False),
    ("matern52", 65, 16, 65, 2, 127, 1e-2, True),
    ("rbf", 130, 17, 64, 15, 1, 1e-6, True),
]
LARGE = dict(kind="matern52", N=256, D=4, F=1024, S=8, m=32768 + 5, noise=1e-2)


@pytest.fixture(scope="module")
def emu_ctx():
    sys.path.insert(0, os.path.join(HERE, "hipemu"))
    import build_emu
    _lib.use_library(build_emu.build())
    ctx = _lib.Context(0)
    assert "hipemu" in ctx.name
    yield ctx
    ctx.close()
    _lib.use_library(None)


@pytest.fixture(scope="module")
def gpu_ctx():
    _lib.use_library(None)
    if _lib.device_count() < 1:
        pytest.skip("no HIP device")
    yield _lib.default_context()


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


class _Worst(object):
    ratio = 0.0


def _bound(orc_row, dev):
    """the value bound of one path over a case's candidates (per candidate)"""
    o = np.abs(np.asarray(orc_row, dtype=np.float64))
    return MU_RTOL * o + MU_ATOL * max(1.0, float(o.max())) + 20.0 * dev


class _Problem(object):
    """one data set, one theta, its draws, and the oracle's values (computed once, shared, read-only)"""

    def __init__(self, kind, N, D, F, S, m, noise, norm, seed=0):
        rs = np.random.RandomState(1000 * seed + 7 * N + D)
        self.kind, self.N, self.D, self.F, self.S, self.m, self.norm = kind, N, D, F, S, m, norm
        self.X = rs.rand(N, D)
        y = np.sin(3.0 * self.X.sum(axis=1) / np.sqrt(D)) + 0.1 * rs.randn(N)
        self.y_mean, self.y_std = (float(y.mean()), float(y.std())) if norm else (0.0, 1.0)
        self.y = (y - self.y_mean) / self.y_std
        self.mean_c = float(self.y.mean())
        self.lnm = np.log(np.linspace(0.3, 0.9, D))
        self.theta = np.concatenate([[np.log(AMP)], self.lnm, [np.log(noise)]])
        self.noise = float(np.exp(self.theta[-1]))
        self.omega, self.phase = draw_features(kind, D, F, rs)
        self.w, self.eps = rs.standard_normal((S, F)), rs.standard_normal((S, N))
        self.Xc = rs.rand(m, D)
        self._orc = None

    def fit(self, ctx):
        g = _lib.DeviceGP(ctx, self.kind, self.N, self.D)
        g.set_data(self.X, self.y)
        g.set_output_transform(self.y_mean, self.y_std)
        g.fit(self.theta, self.mean_c)
        return g

    def paths_of(self, w, eps, dtype):
        return PO.Paths(self.kind, AMP, self.noise, CO.scale(self.X, self.lnm), self.y, self.mean_c, self.omega, self.phase, w,
                        eps, self.y_mean, self.y_std, dtype=dtype)

    def oracle_of(self, w, eps, Xc, dtype):
        return self.paths_of(w, eps, dtype).values(CO.scale(Xc, self.lnm))

    def oracle(self):
        """(long-double values (S, m), dev (S,): the fp64 model's largest deviation per path)"""
        if self._orc is None:
            o = self.oracle_of(self.w, self.eps, self.Xc, PO.LD)
            m64 = self.oracle_of(self.w, self.eps, self.Xc, np.float64)
            dev = np.max(np.abs(m64 - o), axis=1).astype(np.float64)
            o.setflags(write=False)
            self._orc = (o, dev)
        return self._orc


_PROBLEMS = {}


def _problem(*key):
    if key not in _PROBLEMS:
        _PROBLEMS[key] = _Problem(*key)
    return _PROBLEMS[key]


def _check_values(vals, orc, dev, label, worst):
    """every value of every path against the bound -> the failures (the caller prints its figure, then asserts there are none)"""
    fails = []
    for s in range(vals.shape[0]):
        bound = _bound(orc[s], dev[s])
        err = np.abs(vals[s].astype(PO.LD) - orc[s]).astype(np.float64)
        worst.ratio = max(worst.ratio, float(np.max(err / bound)))
        bad = np.flatnonzero(~(err <= bound))
        if bad.size:
            fails.append((label, s, int(bad[0]), float(err[bad[0]]), float(bound[bad[0]])))
    return fails


def _picks_against(argmin, orc, dev, label):
    """per path: the device's pick is the oracle's unless the oracle's best two are closer than the value bound
    -> (cases, excluded)"""
    excluded = 0
    for s in range(orc.shape[0]):
        o = np.asarray(orc[s], dtype=np.float64)
        best = int(PO.np_argmax_neg(o)[0])
        if o.shape[0] > 1:
            second = np.partition(o, 1)[1]
            if second - o[best] < _bound(o, dev[s])[best]:
                excluded += 1
                continue
        assert int(argmin[s]) == best, (label, s, int(argmin[s]), best)
    return orc.shape[0], excluded


# ---- 1. the host recipe (NumPy only) -------------------------------------------------------------------------------------------
def test_features_reproduce_the_kernel():
    """Phi Phi^T against k on 40 scaled points, F = 2048, amp = 1.7, seeds 0 .. 19: within 6 amp / sqrt(F).  Worst observed, in
    units of amp / sqrt(F): 3.9 (matern52), 3.8 (rbf)."""
    amp, F = 1.7, 2048
    for kind in ("matern52", "rbf"):
        worst = 0.0
        for D in (1, 3, 16):
            Xs = np.random.RandomState(50 + D).rand(40, D) * 2.0
            K = CO.kernel(kind, amp, Xs, dtype=np.float64)
            for seed in range(20):
                omega, phase = draw_features(kind, D, F, np.random.RandomState(seed))
                assert omega.shape == (F, D) and phase.shape == (F,) and phase.min() >= 0 and phase.max() < 2 * np.pi
                Phi = PO.features(amp, Xs, omega, phase, dtype=np.float64)
                worst = max(worst, float(np.max(np.abs(Phi @ Phi.T - K))) / (amp / np.sqrt(F)))
        print("%s: max |Phi Phi^T - K| = %.2f amp / sqrt(F)" % (kind, worst))
        assert worst <= 6.0
    with pytest.raises(ValueError, match="stationary"):
        draw_features("fabolas", 3, 8, np.random.RandomState(0))


def test_oracle_mean_is_the_posterior_mean():
    """the rule's mean over 4000 paths (N = 30, D = 2, F = 4096, noise 1e-2; the routine in np.float64) within 5 standard errors
    of the exact posterior mean at 25 points.  Observed: 3.1 standard errors at the worst point."""
    rs = np.random.RandomState(3)
    N, D, F, S = 30, 2, 4096, 4000
    X, Xc = rs.rand(N, D), rs.rand(25, D)
    y = np.sin(4.0 * X.sum(axis=1)) + 0.1 * rs.randn(N)
    lnm, noise, mean = np.log([0.3, 0.5]), 1e-2, float(y.mean())
    Xs, Xcs = CO.scale(X, lnm), CO.scale(Xc, lnm)
    omega, phase = draw_features("matern52", D, F, rs)
    f = PO.Paths("matern52", AMP, noise, Xs, y, mean, omega, phase, rs.standard_normal((S, F)), rs.standard_normal((S, N)),
                 dtype=np.float64).values(Xcs)
    mu = np.asarray(CO.Posterior("matern52", AMP, noise, Xs, y, mean).predict(Xcs)[0], dtype=np.float64)
    se = f.std(axis=0, ddof=1) / np.sqrt(S)
    z = np.abs(f.mean(axis=0) - mu) / se
    print("mean of %d paths against the posterior mean: %.2f standard errors at the worst of %d points" % (S, z.max(), len(z)))
    assert z.max() <= 5.0 and se.min() > 0


# ---- 2. values against the oracle ------------------------------------------------------------------------------------------------
def _check_value_cases(ctx, label):
    worst = _Worst()
    for case in CASES:
        pr = _problem(*case)
        orc, dev = pr.oracle()
        g = pr.fit(ctx)
        p = g.sample_paths(pr.omega, pr.phase, pr.w, pr.eps)
        try:
            r = p.evaluate(pr.Xc)
            assert r.values.shape == (pr.S, pr.m) and r.flags == 0, case
            one = _Worst()
            fails = _check_values(r.values, orc, dev, "%s %r" % (label, case), one)
            print("%s %r: error / bound = %.3g (fp64 model deviates by %.3g)" % (label, case, one.ratio, dev.max()))
            worst.ratio = max(worst.ratio, one.ratio)
            assert not fails, fails
            assert np.array_equal(r.argmin, PO.np_argmax_neg(r.values)), case
            assert _bits(r.min, r.values[np.arange(pr.S), r.argmin]), case
        finally:
            p.close()
            g.close()
    print("%s: value cases, largest error / bound = %.3g" % (label, worst.ratio))
    return worst.ratio


# ---- 3. bit-for-bit invariances ----------------------------------------------------------------------------------------------------
def _check_invariances(ctx, label):
    pr = _problem("matern52", 130, 3, 300, 17, 401, 1e-6, False)
    g = pr.fit(ctx)
    rs = np.random.RandomState(11)
    p = g.sample_paths(pr.omega, pr.phase, pr.w, pr.eps)
    cand = _lib.Candidates(ctx, pr.Xc)
    try:
        base = p.evaluate(cand)
        # the same rows at other positions of a batch of another size
        big = np.concatenate((rs.rand(130, pr.D), pr.Xc[::-1], rs.rand(77, pr.D)))
        rb = p.evaluate(big)
        assert _bits(rb.values[:, 130:130 + pr.m][:, ::-1], base.values)
        assert _bits(p.evaluate(pr.Xc[:77]).values, base.values[:, :77])
        assert _bits(p.evaluate(pr.Xc[200:201]).values, base.values[:, 200:201])
        # several passes through a one-block workspace against the single pass
        ctx.set_tuning("ws_bytes", 128 * 256 * 8)
        try:
            rp = p.evaluate(cand)
            assert cand.chunk() == 128 and pr.m > 3 * 128
            rq = p.evaluate(cand, want_values=False)
        finally:
            ctx.set_tuning("ws_bytes", None)
        assert _bits(rp.values, base.values) and _bits(rp.min, base.min) and np.array_equal(rp.argmin, base.argmin)
        assert _bits(rq.min, base.min) and np.array_equal(rq.argmin, base.argmin) and rq.flags == 0
        # out_values NULL against given
        rn = p.evaluate(cand, want_values=False)
        assert rn.values is None and _bits(rn.min, base.min) and np.array_equal(rn.argmin, base.argmin) and rn.flags == base.flags
        # two calls, two objects from the same draws
        assert _bits(p.evaluate(cand).values, base.values)
        p2 = g.sample_paths(pr.omega, pr.phase, pr.w, pr.eps)
        try:
            assert _bits(p2.evaluate(cand).values, base.values)
        finally:
            p2.close()
        # path 5 alone, and inside 64 paths with other draws around it
        s = 5
        p1 = g.sample_paths(pr.omega, pr.phase, pr.w[s:s + 1], pr.eps[s:s + 1])
        w64, e64 = rs.standard_normal((64, pr.F)), rs.standard_normal((64, pr.N))
        w64[40], e64[40] = pr.w[s], pr.eps[s]
        p64 = g.sample_paths(pr.omega, pr.phase, w64, e64)
        try:
            r1, r64 = p1.evaluate(cand), p64.evaluate(cand)
            assert _bits(r1.values[0], base.values[s]) and _bits(r64.values[40], base.values[s])
            assert r1.argmin[0] == base.argmin[s] == r64.argmin[40] and _bits(r1.min, base.min[s:s + 1])
        finally:
            p1.close()
            p64.close()
    finally:
        cand.close()
        p.close()
        g.close()


# ---- 4. structure --------------------------------------------------------------------------------------------------------------------
def _check_structure(ctx, label):
    pr = _problem("rbf", 130, 3, 64, 2, 129, 1e-2, True)
    g = pr.fit(ctx)
    cand = _lib.Candidates(ctx, pr.Xc)
    try:
        # no draws: the posterior mean, within the mean contract
        p0 = g.sample_paths(pr.omega, pr.phase, np.zeros((2, pr.F)), np.zeros((2, pr.N)))
        try:
            mean, _ = g.predict(cand)
            r0 = p0.evaluate(cand)
            tol = MU_RTOL * np.abs(mean) + MU_ATOL * max(1.0, float(np.abs(mean).max()))
            print("%s: w = 0, eps = 0 against predict's mean: %.3g of the tolerance" % (label, np.max(np.abs(r0.values - mean) / tol)))
            assert np.all(np.abs(r0.values - mean[None, :]) <= tol[None, :]) and _bits(r0.values[0], r0.values[1])
        finally:
            p0.close()
        # a snapshot: other data, another theta, then no GP at all
        p = g.sample_paths(pr.omega, pr.phase, pr.w, pr.eps)
        try:
            before = p.evaluate(cand)
            rs = np.random.RandomState(5)
            g.set_data(rs.rand(pr.N - 20, pr.D), rs.randn(pr.N - 20))
            g.set_output_transform(0.3, 2.0)
            g.fit(pr.theta + 0.4, 0.1)
            assert not _bits(g.sample_paths(pr.omega, pr.phase, pr.w, pr.eps[:, :pr.N - 20]).evaluate(cand).values, before.values)
            after = p.evaluate(cand)
            assert _bits(after.values, before.values) and np.array_equal(after.argmin, before.argmin)
            g.close()
            gone = p.evaluate(cand)
            assert _bits(gone.values, before.values) and _bits(gone.min, before.min)
        finally:
            p.close()
    finally:
        cand.close()
        g.close()


# ---- 5. reduction and protocol -------------------------------------------------------------------------------------------------------
def _check_reduction_and_protocol(ctx, label):
    pr = _problem("matern52", 65, 3, 65, 17, 129, 1e-2, False)
    g = pr.fit(ctx)
    p = g.sample_paths(pr.omega, pr.phase, pr.w, pr.eps)
    other = _lib.Context(0)
    try:
        base = p.evaluate(pr.Xc)
        # ties: every row twice -- the first index
        twice = p.evaluate(np.concatenate((pr.Xc, pr.Xc)))
        assert _bits(twice.values[:, pr.m:], base.values) and np.array_equal(twice.argmin, base.argmin)
        assert np.all(twice.values[np.arange(pr.S), twice.argmin] == twice.values[np.arange(pr.S), twice.argmin + pr.m])
        # a NaN coordinate: NaN in every path there, the pick of every path, the flag
        Xn = pr.Xc.copy()
        Xn[[30, 11], [0, 2]] = np.nan
        rn = p.evaluate(Xn)
        assert np.isnan(rn.values[:, [11, 30]]).all() and np.isnan(rn.values).sum() == 2 * pr.S
        assert _bits(np.delete(rn.values, [11, 30], axis=1), np.delete(base.values, [11, 30], axis=1))
        assert rn.flags == _lib.FLAG_NAN and np.isnan(rn.min).all() and np.all(rn.argmin == 11)
        rq = p.evaluate(Xn, want_values=False)
        assert rq.flags == _lib.FLAG_NAN and np.all(rq.argmin == 11)
        assert p.evaluate(pr.Xc).flags == 0                                        # the flag does not stick
        # refusals of robo_paths_create: the status, a reason, no object
        L = _lib.lib()
        S, F, N, D = 2, 8, pr.N, pr.D
        rs = np.random.RandomState(2)
        om, ph, w, eps = rs.randn(F, D), rs.rand(F), rs.randn(S, F), rs.randn(S, N)
        import ctypes as C

        def create(gp, F_, S_, om_, ph_, w_, eps_, want, null_out=False):
            h = C.c_void_p()
            ptr = lambda a: None if a is None else _lib._arr(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
            st = L.robo_paths_create(gp, F_, S_, ptr(om_), ptr(ph_), ptr(w_), ptr(eps_), None if null_out else C.byref(h))
            assert st == want and not h.value and len(_lib.last_error()) > 0, (st, want, _lib.last_error())
            return _lib.last_error()
        fab = _lib.DeviceGP(ctx, "fabolas", N, D)
        raw = _lib.DeviceGP(ctx, "matern52", N, D)
        try:
            assert "stationary" in create(fab._h, F, S, om, ph, w, eps, _lib.BAD_ARGUMENT)
            create(raw._h, F, S, om, ph, w, eps, _lib.NOT_FITTED)
            big = _lib.PATHS_MAX_FEATURES + 1
            create(g._h, 0, S, om, ph, w, eps, _lib.BAD_ARGUMENT)
            create(g._h, big, S, np.zeros((big, D)), np.zeros(big), np.zeros((S, big)), eps, _lib.BAD_ARGUMENT)
            create(g._h, F, 0, om, ph, w, eps, _lib.BAD_ARGUMENT)
            create(g._h, F, _lib.PATHS_MAX + 1, om, ph, np.zeros((65, F)), np.zeros((65, N)), _lib.BAD_ARGUMENT)
            for k in range(4):
                args = [om, ph, w, eps]
                args[k] = None
                create(g._h, F, S, *args, _lib.BAD_ARGUMENT)
                for v in (np.nan, np.inf, -np.inf):
                    args = [om.copy(), ph.copy(), w.copy(), eps.copy()]
                    args[k].flat[-1] = v
                    create(g._h, F, S, *args, _lib.BAD_ARGUMENT)
            create(None, F, S, om, ph, w, eps, _lib.BAD_ARGUMENT)
            create(g._h, F, S, om, ph, w, eps, _lib.BAD_ARGUMENT, null_out=True)
        finally:
            fab.close()
            raw.close()
        with pytest.raises(_lib.RoboBadShape):
            g.sample_paths(om[:, :2], ph, w, eps)
        with pytest.raises(_lib.RoboBadShape):
            g.sample_paths(om, ph, w, eps[:, :-1])
        # refusals of robo_paths_eval_cand
        cand = _lib.Candidates(ctx, pr.Xc)
        wide = _lib.Candidates(ctx, rs.rand(5, D + 1))
        far = _lib.Candidates(other, pr.Xc[:5])
        try:
            with pytest.raises(_lib.RoboBadShape):
                p.evaluate(wide)
            with pytest.raises(ValueError, match="context"):
                p.evaluate(far)
            mn, am, fl = np.empty(pr.S), np.empty(pr.S, dtype=np.int64), C.c_uint32(0)
            i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))  # noqa: E731
            for a in ((None, cand._h, None, _lib._arr(mn), i64(am), C.byref(fl)),
                      (p._h, None, None, _lib._arr(mn), i64(am), C.byref(fl)),
                      (p._h, cand._h, None, None, i64(am), C.byref(fl)),
                      (p._h, cand._h, None, _lib._arr(mn), None, C.byref(fl)),
                      (p._h, cand._h, None, _lib._arr(mn), i64(am), None)):
                assert L.robo_paths_eval_cand(*a) == _lib.BAD_ARGUMENT and len(_lib.last_error()) > 0
            ok = p.evaluate(cand)
            assert _bits(ok.values, base.values) and ok.flags == 0               # the handles stay usable
        finally:
            for h in (cand, wide, far):
                h.close()
        assert L.robo_paths_destroy(None) == _lib.OK
    finally:
        other.close()
        p.close()
        g.close()


# ---- 6. the class and the front end ------------------------------------------------------------------------------------------------
_BOX = (np.array([-5.0, 0.0]), np.array([10.0, 15.0]))


def _branin(x):
    x = np.asarray(x, dtype=np.float64)
    return float((x[1] - 5.1 / (4 * np.pi ** 2) * x[0] ** 2 + 5.0 / np.pi * x[0] - 6.0) ** 2
                 + 10.0 * (1.0 - 1.0 / (8 * np.pi)) * np.cos(x[0]) + 10.0)


def _data(n, seed):
    rs = np.random.RandomState(seed)
    X = _BOX[0] + (_BOX[1] - _BOX[0]) * rs.rand(n, 2)
    return rs, X, np.array([_branin(x) for x in X]) / 50.0


def _gp_model(normalize_output=True):
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models import GaussianProcess
    rs, X, y = _data(14, 0)
    model = GaussianProcess(2 * Matern52Kernel(np.array([0.5, 0.8]), ndim=2), noise=1e-3, lower=_BOX[0], upper=_BOX[1],
                            normalize_output=normalize_output)
    model.train(X, y, do_optimize=False)
    return rs, model


def _mcmc_model():
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models.gaussian_process_mcmc import GaussianProcessMCMC
    from robo_amd.priors.default_priors import DefaultPrior
    rs, X, y = _data(10, 2)
    kernel = 2 * Matern52Kernel(np.ones(2), ndim=2)
    model = GaussianProcessMCMC(kernel, prior=DefaultPrior(len(kernel) + 1, rng=np.random.RandomState(3)), n_hypers=8,
                                chain_length=4, burnin_steps=2, rng=np.random.RandomState(4), lower=_BOX[0], upper=_BOX[1])
    model.train(X, y)
    return rs, model


def _replay(model, seed, n_paths, n_features, Xc):
    """the draws of ThompsonSampling._draw from the same seed, through the oracle -> (hyper indices, values (S, m), dev (S,))"""
    subs = list(model.models) if hasattr(model, "models") else [model]
    rs = np.random.RandomState(seed)
    idx = np.array([rs.randint(len(subs)) for _ in range(n_paths)]) if len(subs) > 1 else np.zeros(n_paths, dtype=np.int64)
    vals, dev = np.empty((n_paths, Xc.shape[0]), dtype=PO.LD), np.empty(n_paths)
    for i in sorted(set(idx.tolist())):
        sub = subs[i]
        members = np.flatnonzero(idx == i)
        theta = np.asarray(_lib._full_theta(sub.gp, sub._fitted_theta), dtype=np.float64)
        D, N = sub.X.shape[1], sub.X.shape[0]
        omega, phase = draw_features(sub.kernel.kind, D, n_features, rs)
        w, eps = rs.standard_normal((len(members), n_features)), rs.standard_normal((len(members), N))
        Xs, Xcs = CO.scale(sub.X, theta[1:-1]), CO.scale(sub._normalised(Xc), theta[1:-1])
        ym, ys = (sub.y_mean, sub.y_std) if sub.normalize_output else (0.0, 1.0)
        out = [PO.Paths(sub.kernel.kind, float(np.exp(theta[0])), float(np.exp(theta[-1])), Xs, sub.y, float(sub.mean), omega,
                        phase, w, eps, ym, ys, dtype=dt).values(Xcs) for dt in (PO.LD, np.float64)]
        vals[members] = out[0]
        dev[members] = np.max(np.abs(out[1] - out[0]), axis=1).astype(np.float64)
    return idx, vals, dev


def _check_class(ctx, label):
    from robo_amd.acquisition_functions import ThompsonSampling
    from robo_amd.maximizers import RandomSampling
    from robo_amd.maximizers.random_sampling import DeviceRandomSampling
    worst = _Worst()
    cases = excluded = 0
    for (rs, model), n_paths, seed in ((_gp_model(), 8, 21), (_mcmc_model(), 12, 22)):
        acq = ThompsonSampling(model, n_paths=n_paths, n_features=64, rng=np.random.RandomState(seed))
        acq.update(model)
        Xc = _BOX[0] + (_BOX[1] - _BOX[0]) * rs.rand(90, 2)
        vals, mn, am = acq._evaluate(Xc, True)
        idx, orc, dev = _replay(model, seed, n_paths, 64, Xc)
        assert np.array_equal(acq.hyper_index, idx) and (len(set(idx.tolist())) > 1) == hasattr(model, "models")
        assert len(acq._groups) == len(set(idx.tolist()))
        fails = _check_values(vals, orc, dev, "%s class %s" % (label, type(model).__name__), worst)
        print("%s: class %s, largest error / bound so far = %.3g" % (label, type(model).__name__, worst.ratio))
        assert not fails, fails
        c, e = _picks_against(am, orc, dev, label)
        cases, excluded = cases + c, excluded + e
        a = acq.compute(Xc)
        assert a.shape == (90,) and _bits(a, -vals[0]) and acq.argmax(Xc) == int(am[0]) == acq.last_argmax
        assert _bits([acq.last_max], [a[am[0]]]) and int(np.argmax(a)) == int(am[0])
        # a device batch in the normalised box is the same call
        sub = model.models[0] if hasattr(model, "models") else model
        cand = _lib.Candidates(sub.gp.ctx, sub._normalised(Xc))
        try:
            assert _bits(acq.compute(cand), a) and acq.argmax(cand) == int(am[0])
        finally:
            cand.close()
        # update() draws anew
        acq.update(model)
        assert not _bits(acq.compute(Xc), a)
        # q proposals, one per path, distinct
        pts = acq.select_batch(Xc, 5, fantasy="constant_liar", liar="min")
        assert pts.shape == (5, 2) and len(set(acq.last_batch.tolist())) == 5 and _bits(pts, Xc[acq.last_batch])
        # more proposals than paths: redrawn to q paths
        few = ThompsonSampling(model, n_paths=1, n_features=32, rng=np.random.RandomState(1))
        pts = few.select_batch(Xc, 3)
        assert few.n_paths == 3 and pts.shape == (3, 2) and len(set(few.last_batch.tolist())) == 3
        with pytest.raises(NotImplementedError):
            acq.compute(Xc, derivative=True)
        with pytest.raises(NotImplementedError):
            acq.argmax_sharded(None, Xc[:10], 0)
        with pytest.raises(NotImplementedError):
            RandomSampling(acq, _BOX[0], _BOX[1], n_samples=60, shard=True).maximize()
        with pytest.raises(NotImplementedError):
            acq.compute(_lib.CandidateShards([], []))
        sub.devices = [0, 1]
        try:
            for call in (lambda: acq.argmax(Xc), lambda: acq.compute(Xc), lambda: acq.select_batch(Xc, 2)):
                with pytest.raises(NotImplementedError, match="devices"):
                    call()
        finally:
            sub.devices = None
        np.random.seed(4)
        for mk in (lambda: RandomSampling(acq, _BOX[0], _BOX[1], n_samples=60),
                   lambda: DeviceRandomSampling(acq, _BOX[0], _BOX[1], n_samples=128, rng=np.random.RandomState(9))):
            x = mk().maximize()
            assert x.shape == (2,) and np.all(x >= _BOX[0]) and np.all(x <= _BOX[1])
    print("%s: class replay, %d picks, %d excluded as near ties; largest error / bound = %.3g"
          % (label, cases, excluded, worst.ratio))
    assert cases == 20 and excluded <= 1
    # a constructed collision: paths 0 and 1 are the same function -- path 1 takes its best row not yet taken
    rs, model = _gp_model(normalize_output=False)
    acq = ThompsonSampling(model, n_paths=3, n_features=32, rng=np.random.RandomState(5))
    Xc = _BOX[0] + (_BOX[1] - _BOX[0]) * rs.rand(70, 2)
    omega, phase = draw_features("matern52", 2, 32, rs)
    w, eps = rs.standard_normal((3, 32)), rs.standard_normal((3, model.X.shape[0]))
    w[1], eps[1] = w[0], eps[0]
    acq._groups, acq._stale, acq.hyper_index = [(model.gp.sample_paths(omega, phase, w, eps), np.arange(3))], False, np.zeros(3)
    vals, mn, am = acq._evaluate(Xc, True)
    assert am[0] == am[1] and _bits(vals[0], vals[1])
    pts = acq.select_batch(Xc, 3)
    picks = acq.last_batch.tolist()
    order = np.argsort(vals[1], kind="stable")
    assert picks[0] == am[0] == order[0] and picks[1] == order[1] and len(set(picks)) == 3 and _bits(pts, Xc[picks])
    assert picks[2] == [i for i in np.argsort(vals[2], kind="stable") if i not in picks[:2]][0]
    with pytest.raises(ValueError):
        ThompsonSampling(model, n_paths=0)
    with pytest.raises(ValueError):
        ThompsonSampling(model, n_features=_lib.PATHS_MAX_FEATURES + 1)
    return worst.ratio


def _check_front_end(ctx):
    from robo_amd.fmin import bayesian_optimization

    def run(seed, **kw):
        np.random.seed(seed)
        calls = []

        def f(x):
            calls.append(np.array(x))
            return _branin(x)
        kw.setdefault("model_type", "gp")
        res = bayesian_optimization(f, _BOX[0], _BOX[1], acquisition_func="thompson", n_init=3, n_candidates=128,
                                    rng=np.random.RandomState(seed), n_features=64, **kw)
        X = np.array(res["X"])
        assert X.shape[0] == len(calls) and np.all(X >= _BOX[0]) and np.all(X <= _BOX[1]) and np.all(np.isfinite(res["y"]))
        return X
    for maximizer in ("random", "device_random"):
        X = run(1, num_iterations=6, maximizer=maximizer)
        assert X.shape == (6, 2) and len({tuple(x) for x in X}) == 6
        assert _bits(run(1, num_iterations=6, maximizer=maximizer), X)              # reproducible from the seed
        assert not _bits(run(2, num_iterations=6, maximizer=maximizer), X)
    X = run(3, num_iterations=6, maximizer="random", model_type="gp_mcmc", chain_length=4, burnin_steps=2)
    assert X.shape == (6, 2)
    # batch_size = 3: rounds of three proposals, one per path; fantasy and liar are ignored
    X = run(1, num_iterations=9, maximizer="random", batch_size=3, fantasy="constant_liar", liar="max")
    assert X.shape == (9, 2) and len({tuple(x) for x in X}) == 9
    assert _bits(run(1, num_iterations=9, maximizer="random", batch_size=3), X)
    X = run(1, num_iterations=6, maximizer="device_random", batch_size=3)
    assert X.shape == (6, 2) and len({tuple(x) for x in X}) == 6


# ---- the runs ------------------------------------------------------------------------------------------------------------------
def test_values_emu(emu_ctx):
    _check_value_cases(emu_ctx, "interpreter")


def test_invariances_emu(emu_ctx):
    _check_invariances(emu_ctx, "interpreter")


def test_structure_emu(emu_ctx):
    _check_structure(emu_ctx, "interpreter")


def test_reduction_and_protocol_emu(emu_ctx):
    _check_reduction_and_protocol(emu_ctx, "interpreter")


def test_class_emu(emu_ctx):
    _check_class(emu_ctx, "interpreter")


def test_front_end_emu(emu_ctx):
    _check_front_end(emu_ctx)


@pytest.mark.gpu
def test_values_gpu(gpu_ctx):
    _check_value_cases(gpu_ctx, "MI355X")


@pytest.mark.gpu
def test_invariances_and_structure_gpu(gpu_ctx):
    _check_invariances(gpu_ctx, "MI355X")
    _check_structure(gpu_ctx, "MI355X")


@pytest.mark.gpu
def test_reduction_and_protocol_gpu(gpu_ctx):
    _check_reduction_and_protocol(gpu_ctx, "MI355X")


@pytest.mark.gpu
def test_class_and_front_end_gpu(gpu_ctx):
    _check_class(gpu_ctx, "MI355X")
    _check_front_end(gpu_ctx)


@pytest.mark.gpu
def test_fused_large_gpu(gpu_ctx):
    """N = 256, D = 4, F = 1024, S = 8, m = 32 773: 514 tiles in one pass (more than two per CU), then three passes through a
    smaller workspace.  Every value of 512 fixed rows and of the 8 picked rows against the oracle; the picks against the
    oracle's on the full set."""
    sz = LARGE
    pr = _Problem(sz["kind"], sz["N"], sz["D"], sz["F"], sz["S"], sz["m"], sz["noise"], True, seed=4)
    g = pr.fit(gpu_ctx)
    p = g.sample_paths(pr.omega, pr.phase, pr.w, pr.eps)
    cand = _lib.Candidates(gpu_ctx, pr.Xc)
    worst = _Worst()
    try:
        r = p.evaluate(cand)
        assert r.flags == 0 and np.array_equal(r.argmin, PO.np_argmax_neg(r.values))
        gpu_ctx.set_tuning("ws_bytes", 12288 * 384 * 8)
        try:
            rp = p.evaluate(cand)
            assert cand.chunk() == 12288
            rq = p.evaluate(cand, want_values=False)
        finally:
            gpu_ctx.set_tuning("ws_bytes", None)
        assert _bits(rp.values, r.values) and np.array_equal(rp.argmin, r.argmin) and _bits(rq.min, r.min)
        assert np.array_equal(rq.argmin, r.argmin)
        # the oracle on the full set, in slices of 4096 rows
        exact, Xcs = pr.paths_of(pr.w, pr.eps, PO.LD), CO.scale(pr.Xc, pr.lnm)
        orc = np.concatenate([exact.values(Xcs[c:c + 4096]) for c in range(0, pr.m, 4096)], axis=1)
        m64 = pr.oracle_of(pr.w, pr.eps, pr.Xc, np.float64)
        dev = np.max(np.abs(m64 - orc), axis=1).astype(np.float64)
        rows = np.unique(np.concatenate((np.random.RandomState(8).choice(pr.m, 512, replace=False), r.argmin)))
        for s in range(pr.S):
            bound = _bound(orc[s], dev[s])[rows]
            err = np.abs(r.values[s][rows].astype(PO.LD) - orc[s][rows]).astype(np.float64)
            worst.ratio = max(worst.ratio, float(np.max(err / bound)))
            assert np.all(err <= bound), (s, float(np.max(err / bound)))
        cases, excluded = _picks_against(r.argmin, orc, dev, "fused large")
        print("MI355X: fused large, largest error / bound = %.3g; %d picks, %d excluded as near ties"
              % (worst.ratio, cases, excluded))
        assert excluded <= 1
    finally:
        cand.close()
        p.close()
        g.close()
