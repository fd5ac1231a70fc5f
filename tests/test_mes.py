"""Max-value entropy search (robo_amd/csrc/mes.hip: robo_mes_eval_cand, robo_mes_eval_marginal_cand,
robo_mes_sample_min_moments, robo_mes_eval_moments; the MES class and the "mes" front end) against tests/mes_oracle.py.

CPU: through the interpreter (tests/hipemu).  -m gpu: the same checks at the same small shapes on the MI355X, plus the
fused form at N = 256, D = 16, M = 65 539 (more than 256 partial blocks of the argmax, 513 of the F pass, a two-block
factor).

The quantile bound.  The search's contract is a bracket no wider than W = max((w_hi - w_lo) 2^-46, 4 ulp); the device
evaluates F in fp64, so the bracket it closes is that of a slightly different function.  Each returned w_p must satisfy
F_ld(w_p - t) <= log p <= F_ld(w_p + t) in the longdouble oracle with t = W + MES_F_ROUNDING_REL (w_hi - w_lo).
MES_F_ROUNDING_REL is the measured effect of F's fp64 rounding times a head-room of about 10.  The device's own F is not
exported, so the figure is a PROXY: it is measured on an fp64 restatement that shares the device's order of additions
but takes log Phi from scipy's log_ndtr, not from the erfcx / log1p forms of kern_math.h.  (The term is about 50 times
smaller than W; what the device itself shows is the second pair of lines.)  Measured here as
|F64(w_p) - F_ld(w_p)| / F_ld'(w_p) / (w_hi - w_lo), F64 being the fp64 restatement of the device's sum (scipy's log_ndtr,
128 candidates per partial in index order, partials in block order), max over M = 1, 7, 300 and the three quantiles:
    fp64 restatement:                2.8e-17
What a run itself shows is the distance of the returned w_p from the longdouble root, in units of W (<= 1/2 from the
contract alone, anything beyond it is rounding):
    interpreter:                     max |w_p - root_ld| / W = 0.25     (M = 1, p = 1/2)
    MI355X:                          max |w_p - root_ld| / W = 0.25     (M = 1, p = 1/2)

y* is held to the 4 ulp of its own value (against the host's -(a - b log(-log u)) on the device's (a, b)); measured
distance over the 24 draws of the sampling cases: interpreter 0 ulp everywhere, MI355X at most 1 ulp (one draw).
"""
import os
import sys

import numpy as np
import pytest

from robo_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mes_oracle as MO  # noqa: E402
from _tol import ACQ_RTOL  # noqa: E402

MES_F_ROUNDING_REL = 3e-16       # about 10 x the 2.8e-17 measured above

SMALL = dict(N=80, D=3, M=400)
LARGE = dict(N=256, D=16, M=65539)
KINDS = ("matern52", "rbf", "fabolas")


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


# ---- a. the element-wise half ------------------------------------------------------------------------------------------
def _gamma_case(m, K, seed):
    """(mu, v, y*) whose gamma of draw 0 is a grid over [-30, 40]"""
    rs = np.random.RandomState(seed)
    ystar = np.linspace(-0.5, 0.5, K) if K > 1 else np.array([0.1])
    v = 10 ** rs.uniform(-4, 0, m)
    gam = np.linspace(-30.0, 40.0, m)
    return ystar[0] + gam * np.sqrt(v), v, ystar


def _check_elementwise(ctx):
    worst = 0.0
    for K in (1, 37):
        for m in (1, 257):
            mu, v, ystar = _gamma_case(m, K, 10 * K + m)
            al, mx, am, fl = _lib.mes_from_moments(ctx, mu, v, ystar)
            ref = MO.values(mu, v, ystar)
            with np.errstate(invalid="ignore"):
                worst = max(worst, float(np.nanmax(np.abs(al - ref) / np.abs(ref))))
            np.testing.assert_allclose(al, ref, rtol=ACQ_RTOL, atol=0)
            assert fl == 0 and am == MO.np_argmax(al) and np.array([mx]).tobytes() == al[am:am + 1].tobytes()
    print("element-wise half: max relative difference to the oracle %.3e" % worst)
    mu, v, ystar = _gamma_case(257, 37, 5)
    # a value tied between two indices returns the first
    i = MO.np_argmax(MO.values(mu, v, ystar))
    j = 200 if i != 200 else 100
    mu[j], v[j] = mu[i], v[i]
    al, mx, am, fl = _lib.mes_from_moments(ctx, mu, v, ystar)
    assert al[i] == al[j] == mx and am == min(i, j) and fl == 0
    # v = 0: value 0 with the flag
    v[7] = 0.0
    al, mx, am, fl = _lib.mes_from_moments(ctx, mu, v, ystar)
    assert al[7] == 0.0 and fl == _lib.FLAG_ZERO_SIGMA and am == min(i, j)
    np.testing.assert_allclose(al, MO.values(mu, v, ystar), rtol=ACQ_RTOL, atol=0)
    # a NaN mean: NaN, the flag, and it wins the argmax
    mu[250] = np.nan
    al, mx, am, fl = _lib.mes_from_moments(ctx, mu, v, ystar)
    assert np.isnan(al[250]) and np.isnan(mx) and am == 250 and fl == _lib.FLAG_ZERO_SIGMA | _lib.FLAG_NAN
    assert np.isnan(al).sum() == 1
    # gamma = 5000 gives exactly 0 (exp underflows to 0, 0 * gamma counts as 0)
    s = np.sqrt(np.array([1e-4, 0.25]))
    al, mx, am, fl = _lib.mes_from_moments(ctx, 0.3 + 5000.0 * s, s * s, np.array([0.3]))
    assert _bits(al, np.zeros(2)) and am == 0 and fl == 0
    for K in (0, 129):
        with pytest.raises(ValueError):
            _lib.mes_from_moments(ctx, mu, v, np.zeros(K))


# ---- b. the sampling half ----------------------------------------------------------------------------------------------
def _sampling_case(M, seed):
    rs = np.random.RandomState(seed)
    mu = np.sin(3 * rs.rand(M)) + 0.3 * rs.randn(M)
    v = 10 ** rs.uniform(-6, 0, M)
    if M == 7:
        v[3] = 0.0
    u = np.concatenate([rs.rand(6), [1e-12, 1 - 1e-12]])
    return mu, v, u


def _f64_device_order(w, mu, var):
    """F(w) in fp64 with the device's order of additions (128 candidates per partial, partials in block order)"""
    from scipy.special import log_ndtr
    s = np.sqrt(var)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(s == 0.0, np.where(w < -mu, -np.inf, 0.0), log_ndtr((w + mu) / np.where(s == 0.0, 1.0, s)))
    parts = [np.cumsum(np.concatenate(([0.0], t[b:b + 128])))[-1] for b in range(0, len(t), 128)]
    return np.cumsum(np.concatenate(([0.0], parts)))[-1]


def _check_quantiles(mu, v, gum, label, ps=MO.P):
    """w_lo / w_hi bit for bit; every w_p within t of the longdouble root; -> (max |w_p - root| / W, max rounding effect)"""
    lo, hi = MO.bracket(mu, v)
    assert _bits(gum[:2], [lo, hi]), (label, gum[:2], lo, hi)
    W = MO.contract_width(lo, hi)
    t = W + MES_F_ROUNDING_REL * (hi - lo)
    worst_w = worst_r = 0.0
    for p in ps:
        w = gum[2 + MO.P.index(p)]
        logp = np.log(MO.LD(p))
        below, above = MO.F_ld(MO.LD(w) - t, mu, v), MO.F_ld(MO.LD(w) + t, mu, v)
        if hi > lo:
            root = MO.root_ld(p, mu, v)
            worst_w = max(worst_w, float(abs(MO.LD(w) - root)) / W)
            h = MO.LD(1e-6) * (hi - lo)
            slope = (MO.F_ld(MO.LD(w) + h, mu, v) - MO.F_ld(MO.LD(w) - h, mu, v)) / (2 * h)
            if np.isfinite(slope) and slope > 0:
                err = abs(MO.LD(_f64_device_order(w, mu, v)) - MO.F_ld(w, mu, v))
                worst_r = max(worst_r, float(err / slope / (hi - lo)))
        print("%s p = %.2f: w_p = %.17g, F_ld(w_p - t) - log p = %.3e, F_ld(w_p + t) - log p = %.3e"
              % (label, p, w, float(below - logp), float(above - logp)))
        assert below <= logp <= above, (label, p, w, float(below - logp), float(above - logp))
    return worst_w, worst_r


def _check_gumbel_and_draws(gum, ys, u, clamp, eta, label):
    """a, b and y* follow from the device's OWN quantiles to 4 ulp of each result.  -> the largest distance of a y*, in ulp"""
    a, b = MO.gumbel_from_quantiles(*gum[2:5])
    assert abs(gum[5] - a) <= 4 * np.spacing(abs(a)) and abs(gum[6] - b) <= 4 * np.spacing(abs(b)), (label, gum, a, b)
    want = MO.draws(gum[5], gum[6], u, clamp, eta)
    ulps = np.abs(ys - want) / np.spacing(np.abs(want))
    print("%s: y* against the host's expression on the device's (a, b): %s ulp" % (label, np.array2string(ulps, precision=2)))
    assert np.all(ulps <= 4), (label, ys, want, ulps)
    return float(ulps.max())


def _check_sampling(ctx, label):
    worst_w = worst_r = worst_y = 0.0
    for M, seed in ((1, 1), (7, 2), (300, 3)):
        mu, v, u = _sampling_case(M, seed)
        ys, gum = _lib.mes_sample_min(ctx, mu, v, u, clamp=False, diagnostics=True)
        w, r = _check_quantiles(mu, v, gum, "%s M = %d" % (label, M))
        worst_w, worst_r = max(worst_w, w), max(worst_r, r)
        worst_y = max(worst_y, _check_gumbel_and_draws(gum, ys, u, False, 0.0, "%s M = %d" % (label, M)))
        assert ys.shape == (8,) and np.all(np.isfinite(ys)) and ys[6] > ys[:6].max() and ys[7] < ys[:6].min()
        eta = float(np.sort(ys)[3])                                   # clamps the upper half of the draws
        yc, gc = _lib.mes_sample_min(ctx, mu, v, u, clamp=True, eta=eta, diagnostics=True)
        assert _bits(gc, gum) and _bits(yc, np.minimum(ys, eta)) and (yc == eta).sum() >= 4
        y2, g2 = _lib.mes_sample_min(ctx, mu, v, u, clamp=False, diagnostics=True)
        assert _bits(y2, ys) and _bits(g2, gum)                       # two calls, the same bits
    print("%s: max |w_p - root_ld| / W = %.3g, max effect of F's fp64 rounding / (w_hi - w_lo) = %.3e, max y* distance %.2f ulp"
          % (label, worst_w, worst_r, worst_y))
    mu, v, u = _sampling_case(7, 2)
    for bad in (0.0, 1.0, -0.5, np.nan):
        ub = u.copy()
        ub[2] = bad
        with pytest.raises(ValueError):
            _lib.mes_sample_min(ctx, mu, v, ub)
    for K in (0, 129):
        with pytest.raises(ValueError):
            _lib.mes_sample_min(ctx, mu, v, np.full(K, 0.5))
    for arr in (mu, v):                                               # a NaN moment in the sampling half
        a = arr.copy()
        a[1] = np.nan
        with pytest.raises(ValueError):
            _lib.mes_sample_min(ctx, a if arr is mu else mu, a if arr is v else v, u)


# ---- c. - e. the fused forms -------------------------------------------------------------------------------------------
def _theta(D, ls2, noise=1e-2, kind="matern52"):
    if kind == "fabolas":
        ls2 = ls2 if np.ndim(ls2) == 0 else np.asarray(ls2)[:D - 1]
        return np.concatenate([[0.0], np.log(np.broadcast_to(ls2, (D - 1,))), [np.log(0.5), np.log(0.8)], [np.log(noise)]])
    return np.concatenate([[0.0], np.log(np.broadcast_to(ls2, (D,))), [np.log(noise)]])


def _ls2(D):
    return np.array([0.3, 0.5, 0.8, 0.4, 0.6])[:D] if D <= 5 else 0.25 * D


def _data(N, D, seed):
    rs = np.random.RandomState(seed)
    X = rs.rand(N, D)
    y = np.sin(3 * X.sum(axis=1) / np.sqrt(D / 3.0)) + 0.1 * rs.randn(N)
    return rs, X, y


def _fit(ctx, kind, theta, X, y):
    g = _lib.DeviceGP(ctx, kind, X.shape[0], X.shape[1])
    g.set_data(X, y)
    g.fit(theta, float(np.mean(y)))
    return g


def _check_fused_result(ctx, g, cand, eta, u, r, label):
    mean, var = g.predict(cand)
    assert _bits(r.trace[:, 0], mean) and _bits(r.trace[:, 1], var), label
    ys, gum = _lib.mes_sample_min(ctx, mean, var, u, True, eta, diagnostics=True)
    assert _bits(r.ystar, ys) and _bits(r.gumbel, gum), label
    vals, mx, am, fl = _lib.mes_from_moments(ctx, mean, var, r.ystar)
    assert _bits(r.values, vals) and _bits([r.max], [mx]) and r.argmax == am and r.flags == fl, label
    ref = MO.values(mean, var, r.ystar)
    top = np.nanmax(ref)
    assert ref[r.argmax] >= top - ACQ_RTOL * abs(top), (label, r.argmax, ref[r.argmax], top)
    return mean, var


def _check_fused(ctx, sz, kinds, label):
    for kind in kinds:
        rs, X, y = _data(sz["N"], sz["D"], 0)
        g = _fit(ctx, kind, _theta(sz["D"], _ls2(sz["D"]), kind=kind), X, y)
        cand = _lib.Candidates(ctx, rs.rand(sz["M"], sz["D"]))
        try:
            eta, u = float(y.min()), rs.rand(10)
            r = g.mes(eta, cand, u, clamp=True, diagnostics=True)
            mean, var = _check_fused_result(ctx, g, cand, eta, u, r, "%s %s" % (label, kind))
            r2 = g.mes(eta, cand, u, clamp=True, diagnostics=True)
            for a, b in ((r.values, r2.values), (r.ystar, r2.ystar), (r.gumbel, r2.gumbel), (r.trace, r2.trace),
                         ([r.max, r.argmax, r.flags], [r2.max, r2.argmax, r2.flags])):
                assert _bits(a, b), (label, kind)
            r3 = g.mes(eta, cand, u, clamp=True, want_values=False)      # only the maximiser crosses
            assert r3.values is None and r3.argmax == r.argmax and _bits([r3.max], [r.max]) and _bits(r3.ystar, r.ystar)
            w, _ = _check_quantiles(mean, var, r.gumbel, "%s %s M = %d" % (label, kind, sz["M"]), ps=(0.5,))
            print("%s %s: argmax %d, max %.6g, |w_1/2 - root_ld| / W = %.3g" % (label, kind, r.argmax, r.max, w))
        finally:
            cand.close()
            g.close()


def _check_fused_errors(ctx):
    rs, X, y = _data(40, 3, 1)
    g = _fit(ctx, "matern52", _theta(3, _ls2(3)), X, y)
    raw = _lib.DeviceGP(ctx, "matern52", 40, 3)
    cand = _lib.Candidates(ctx, rs.rand(50, 3))
    try:
        for u in (np.array([0.5, 0.0]), np.array([1.0]), np.zeros(0), np.full(129, 0.5)):
            with pytest.raises(ValueError):
                g.mes(0.0, cand, u)
        with pytest.raises(ValueError):
            raw.mes(0.0, cand, np.array([0.5]))                            # not fitted
    finally:
        cand.close()
        raw.close()
        g.close()


def _check_marginal(ctx, sz, label, S=3):
    rs, X, y = _data(sz["N"], sz["D"], 11)
    gps = []
    for s in range(S):
        theta = _theta(sz["D"], _ls2(sz["D"]) * (0.8 + 0.2 * s), noise=1e-2 * (1 + s))
        theta[0] = 0.1 * s
        gps.append(_fit(ctx, "matern52", theta, X, y))
    etas = np.array([y.min() - 0.05 * s for s in range(S)])
    cand = _lib.Candidates(ctx, rs.rand(sz["M"], sz["D"]))
    try:
        u = rs.rand(S, 10)
        rm = _lib.mes_marginal(gps, etas, cand, u, clamp=True, diagnostics=True)
        total = None
        for s, g in enumerate(gps):
            r = g.mes(etas[s], cand, u[s], clamp=True, diagnostics=True)
            _check_fused_result(ctx, g, cand, etas[s], u[s], r, "%s sample %d" % (label, s))
            assert _bits(rm.ystar[s], r.ystar) and _bits(rm.gumbel[s], r.gumbel) and _bits(rm.trace[s], r.trace), (label, s)
            total = r.values if total is None else total + r.values
        assert len({rm.ystar[s].tobytes() for s in range(S)}) == S       # every sample has its own minima
        assert _bits(rm.values, total / S), label
        assert rm.argmax == MO.np_argmax(rm.values) and _bits([rm.max], [rm.values[rm.argmax]])
        rm2 = _lib.mes_marginal(gps, etas, cand, u, clamp=True, want_values=False)
        assert rm2.argmax == rm.argmax and _bits([rm2.max], [rm.max]) and _bits(rm2.ystar, rm.ystar)
    finally:
        cand.close()
        for g in gps:
            g.close()


def _check_shape_change(ctx):
    """one live handle through the state-block shapes K = 3 -> K = 7 -> two samples -> K = 3: every reallocation gives the
    bits of a handle that never held another shape (N = 22, D = 2, 40 candidates: every array of the block is non-empty,
    the odd K puts every later array at an odd multiple of 8 bytes)"""
    rs, X, y = _data(22, 2, 5)
    live, fresh_one, fresh_two = gps = [_fit(ctx, "matern52", _theta(2, _ls2(2)), X, y) for _ in range(3)]
    gps.append(_fit(ctx, "matern52", _theta(2, _ls2(2) * 1.2, noise=3e-2), X, y))      # the marginal form's second sample
    cand = _lib.Candidates(ctx, rs.rand(40, 2))
    eta, u = float(y.min()), rs.rand(2, 7)

    def one(g, K):
        return g.mes(eta, cand, u[0, :K], clamp=True, diagnostics=True)

    def two(g):
        return _lib.mes_marginal([g, gps[3]], np.array([eta, eta - 0.05]), cand, u, clamp=True, diagnostics=True)

    try:
        first, more, both, again = one(live, 3), one(live, 7), two(live), one(live, 3)
        for a, b in ((first, again), (more, one(fresh_one, 7)), (both, two(fresh_two))):
            for p, r in ((a.values, b.values), (a.ystar, b.ystar), (a.gumbel, b.gumbel), (a.trace, b.trace),
                         ([a.max, a.argmax, a.flags], [b.max, b.argmax, b.flags])):
                assert _bits(p, r)
    finally:
        cand.close()
        for g in gps:
            g.close()


# ---- f. host classes and the front end ----------------------------------------------------------------------------------
def _branin(x):
    a, b, c, r, s, t = 1.0, 5.1 / (4 * np.pi ** 2), 5.0 / np.pi, 6.0, 10.0, 1.0 / (8 * np.pi)
    return float(a * (x[1] - b * x[0] ** 2 + c * x[0] - r) ** 2 + s * (1 - t) * np.cos(x[0]) + s)


_BOX = (np.array([-5.0, 0.0]), np.array([10.0, 15.0]))


class _QuadraticModel(object):
    """not a GP: predict() alone (the moments path)"""

    def __init__(self, shift=0.0):
        self.lower, self.upper = _BOX
        self.X = _BOX[0] + (_BOX[1] - _BOX[0]) * np.random.RandomState(0).rand(5, 2)
        self.shift = shift

    def predict(self, X):
        X = np.asarray(X, dtype=np.float64)
        z = (X - self.lower) / (self.upper - self.lower)
        return ((z - 0.4) ** 2).sum(axis=1) + self.shift, 0.01 + 0.05 * z[:, 0] ** 2

    def get_incumbent(self):
        m, _ = self.predict(self.X)
        return self.X[np.argmin(m)], float(m.min())


def _gp_model(seed=0, n=12):
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models import GaussianProcess
    rs = np.random.RandomState(seed)
    X = _BOX[0] + (_BOX[1] - _BOX[0]) * rs.rand(n, 2)
    y = np.array([_branin(x) for x in X])
    model = GaussianProcess(Matern52Kernel(np.array([0.5, 0.5]), ndim=2), noise=1e-3, lower=_BOX[0], upper=_BOX[1])
    model.train(X, y, do_optimize=False)
    return rs, model


def _check_class_moments_path(ctx):
    from robo_amd.acquisition_functions import MES
    model = _QuadraticModel()
    acq = MES(model, n_samples=6, n_grid=300, rng=np.random.RandomState(1))
    Xc = _BOX[0] + (_BOX[1] - _BOX[0]) * np.random.RandomState(2).rand(64, 2)
    a = acq.compute(Xc)
    ys = acq.sampled_minima().copy()
    assert a.shape == (64,) and np.all(np.isfinite(a)) and ys.shape == (6,) and np.all(ys <= model.get_incumbent()[1])
    np.testing.assert_allclose(a, MO.values(*model.predict(Xc), ystar=ys), rtol=ACQ_RTOL, atol=0)
    assert _bits(acq(Xc), a) and _bits(acq.sampled_minima(), ys)          # stable between two calls
    acq.update(_QuadraticModel(shift=0.7))
    b = acq.compute(Xc)
    assert not _bits(acq.sampled_minima(), ys) and not _bits(a, b)        # ... and new after update()
    with pytest.raises(NotImplementedError):
        acq.compute(Xc, derivative=True)
    i = acq.argmax(Xc)                                                     # moments path: both halves on X itself
    m, v = acq.model.predict(Xc)
    assert i == MO.np_argmax(_lib.mes_from_moments(ctx, m, v, acq.last_ystar)[0]) == acq.last_argmax
    with pytest.raises(ValueError):
        MES(model, n_samples=129)
    with pytest.raises(TypeError):
        acq.refine(Xc)
    with pytest.raises(TypeError):
        acq.select_batch(Xc, 2)


def _check_class_gp(ctx):
    from robo_amd.acquisition_functions import MES
    from robo_amd.maximizers import RandomSampling
    from robo_amd.maximizers.random_sampling import DeviceRandomSampling, DeviceSobolSampling
    rs, model = _gp_model()
    acq = MES(model, n_samples=5, n_grid=200, rng=np.random.RandomState(3))
    acq.update(model)
    Xc = _BOX[0] + (_BOX[1] - _BOX[0]) * rs.rand(150, 2)
    a = acq.compute(Xc)
    m, v = model.predict(Xc)
    np.testing.assert_allclose(a, MO.values(m, v, acq.sampled_minima()), rtol=ACQ_RTOL, atol=0)
    assert _bits(acq.compute(Xc), a)
    i = acq.argmax(Xc)
    assert acq.last_ystar.shape == (5,) and np.all(acq.last_ystar <= model.get_incumbent()[1])
    vals = _lib.mes_from_moments(ctx, m, v, acq.last_ystar)[0]
    assert i == MO.np_argmax(vals) == acq.last_argmax and _bits([acq.last_max], [vals[i]])
    cand = _lib.Candidates(model.gp.ctx, model._normalised(Xc))
    try:
        acq.rng = np.random.RandomState(8)
        j = acq.argmax(cand)
        acq.rng = np.random.RandomState(8)
        assert j == acq.argmax(Xc)                                         # a device batch is the same call
    finally:
        cand.close()
    lo, hi = _BOX
    for mk in (lambda: RandomSampling(acq, lo, hi, n_samples=100), lambda: DeviceRandomSampling(acq, lo, hi, n_samples=200,
               rng=np.random.RandomState(9)), lambda: DeviceSobolSampling(acq, lo, hi, n_samples=128, seed=4)):
        x = mk().maximize()
        assert x.shape == (2,) and np.all(x >= lo) and np.all(x <= hi)
    # multi-device and rank-sharded use: out of scope, said plainly
    model.devices = [0, 1]
    try:
        for call in (lambda: acq.argmax(Xc), lambda: acq.compute(Xc), lambda: (acq.update(model), acq.compute(Xc))):
            with pytest.raises(NotImplementedError):
                call()
    finally:
        model.devices = None
    with pytest.raises(NotImplementedError):
        acq.argmax_sharded(None, Xc[:10], 0)
    _check_shard_refusal(acq, model)
    # a device batch handed to compute() needs the normalised box to be the model's input space
    cand = _lib.Candidates(model.gp.ctx, model._normalised(Xc))
    try:
        assert _bits(acq.compute(cand), acq.compute(lo + (hi - lo) * cand.points()))
        model.normalize_input = False
        try:
            with pytest.raises(TypeError):
                acq.compute(cand)
        finally:
            model.normalize_input = True
    finally:
        cand.close()


def _check_shard_refusal(acq, model):
    """shard=True on every sampling maximiser, in a (pretended) world of two ranks: refused before a candidate is drawn, a
    collective is joined or the acquisition is called"""
    from robo_amd import sharding
    from robo_amd.maximizers import RandomSampling
    from robo_amd.maximizers.random_sampling import DeviceRandomSampling, DeviceSobolSampling
    lo, hi = _BOX
    inner = getattr(acq, "acquisition_func", acq)
    calls = []
    real = sharding.dist_info, type(acq).argmax, type(inner).argmax_sharded
    sharding.dist_info = lambda: (None, 0, 2)
    type(acq).argmax = lambda self, X: calls.append("argmax") or 0
    type(inner).argmax_sharded = lambda self, *a: calls.append("argmax_sharded") or 0
    state = np.random.get_state()
    try:
        for mk in (lambda: RandomSampling(acq, lo, hi, n_samples=50, shard=True),
                   lambda: DeviceRandomSampling(acq, lo, hi, n_samples=64, rng=np.random.RandomState(1), shard=True),
                   lambda: DeviceSobolSampling(acq, lo, hi, n_samples=64, seed=2, shard=True)):
            mx = mk()
            with pytest.raises(NotImplementedError, match="shard"):
                mx.maximize()
        assert not calls
        assert np.random.get_state()[1].tobytes() == state[1].tobytes()        # nothing was drawn either
    finally:
        sharding.dist_info, type(acq).argmax, type(inner).argmax_sharded = real


def _check_class_marginal(ctx):
    from robo_amd.acquisition_functions import MES
    from robo_amd.acquisition_functions.marginalization import MarginalizationGPMCMC
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models.gaussian_process_mcmc import GaussianProcessMCMC
    from robo_amd.priors.default_priors import DefaultPrior
    rs = np.random.RandomState(2)
    X = _BOX[0] + (_BOX[1] - _BOX[0]) * rs.rand(14, 2)
    y = np.array([_branin(x) for x in X]) / 50.0
    kernel = 2 * Matern52Kernel(np.ones(2), ndim=2)
    model = GaussianProcessMCMC(kernel, prior=DefaultPrior(len(kernel) + 1, rng=np.random.RandomState(3)), n_hypers=8,
                                chain_length=6, burnin_steps=4, rng=np.random.RandomState(4), lower=_BOX[0], upper=_BOX[1])
    model.train(X, y)
    acq = MarginalizationGPMCMC(MES(model, n_samples=4, n_grid=150, rng=np.random.RandomState(5)))
    acq.update(model)
    assert acq._mes_native()
    Xc = _BOX[0] + (_BOX[1] - _BOX[0]) * rs.rand(120, 2)
    a = acq.compute(Xc)
    S = len(acq.estimators)
    assert acq.last_ystar.shape == (S, 4) and _bits(acq.compute(Xc), a)
    # the generic per-estimator mean with the same y*
    generic = np.mean([e.compute(Xc) for e in acq.estimators], axis=0)
    np.testing.assert_allclose(a, generic, rtol=ACQ_RTOL, atol=0)
    i = acq.argmax(Xc)
    per = [_lib.mes_from_moments(ctx, *e.model.predict(Xc), ystar=acq.last_ystar[s])[0] for s, e in enumerate(acq.estimators)]
    mean = np.sum(per, axis=0) / S
    top = mean.max()
    assert mean[i] >= top - ACQ_RTOL * abs(top) and acq.last_argmax == i
    np.testing.assert_allclose(acq.last_max, mean[i], rtol=ACQ_RTOL, atol=0)
    acq.update(model)
    assert all(e._ystar is None for e in acq.estimators)
    acq.sample_shard = True
    try:
        with pytest.raises(NotImplementedError):
            acq.compute(Xc)
    finally:
        acq.sample_shard = False
    model.devices = [0, 1]
    try:
        with pytest.raises(NotImplementedError):
            acq.argmax(Xc)
    finally:
        model.devices = None
    with pytest.raises(TypeError):
        acq.refine(Xc)
    with pytest.raises(TypeError):
        acq.select_batch(Xc, 2)
    _check_shard_refusal(acq, model)


def _bo(model_type, seed=3, **kw):
    from robo_amd.fmin import bayesian_optimization
    np.random.seed(seed)
    calls = []

    def f(x):
        calls.append(np.array(x))
        return _branin(x)
    res = bayesian_optimization(f, _BOX[0], _BOX[1], num_iterations=6, maximizer="random", acquisition_func="mes",
                                model_type=model_type, n_init=3, rng=np.random.RandomState(seed), n_candidates=200, **kw)
    return res, np.array(calls)


def _check_front_end(ctx):
    for model_type, kw in (("gp", {}), ("gp_mcmc", dict(chain_length=6, burnin_steps=4))):
        a, ca = _bo(model_type, **kw)
        b, cb = _bo(model_type, **kw)
        assert ca.shape == (6, 2) and np.all(np.isfinite(ca)) and np.all(np.isfinite(a["y"])) and np.isfinite(a["f_opt"])
        assert np.all(ca >= _BOX[0]) and np.all(ca <= _BOX[1])              # every proposal inside the box
        assert _bits(ca, cb) and _bits(a["y"], b["y"]) and _bits(a["x_opt"], b["x_opt"])   # identical for identical rng
    from robo_amd.fmin import bayesian_optimization
    with pytest.raises(ValueError):
        bayesian_optimization(_branin, _BOX[0], _BOX[1], num_iterations=3, acquisition_func="mes2")


# ---- the interpreter runs ----------------------------------------------------------------------------------------------
def _run(checks, ctx):
    import traceback
    failed = []
    for name, fn in checks:                      # every item runs and is reported, whatever the earlier ones did
        try:
            fn(ctx)
            print("item ok: " + name)
        except Exception:                        # noqa: BLE001
            failed.append(name)
            print("item FAILED: %s\n%s" % (name, traceback.format_exc()))
    assert not failed, failed


_DEVICE_CHECKS = [("a element-wise half", _check_elementwise),
                  ("b sampling half", lambda c: _check_sampling(c, "sampling")),
                  ("c fused", lambda c: _check_fused(c, SMALL, KINDS, "fused")),
                  ("c fused argument errors", _check_fused_errors),
                  ("d marginal", lambda c: _check_marginal(c, SMALL, "marginal")),
                  ("shape change on a live handle", _check_shape_change)]
_CLASS_CHECKS = [("f moments path", _check_class_moments_path), ("f GP model", _check_class_gp),
                 ("f marginalised", _check_class_marginal), ("f front end", _check_front_end)]


def test_device_checks_emu(emu_ctx):
    _run(_DEVICE_CHECKS, emu_ctx)


def test_classes_and_front_end_emu(emu_ctx):
    _run(_CLASS_CHECKS, emu_ctx)


# ---- the MI355X ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_checks_gpu(gpu_ctx):
    _run(_DEVICE_CHECKS, gpu_ctx)


@pytest.mark.gpu
def test_classes_and_front_end_gpu(gpu_ctx):
    _run(_CLASS_CHECKS, gpu_ctx)


@pytest.mark.gpu
def test_fused_large_gpu(gpu_ctx):
    """e. the reduction's second level (257 partial blocks of the argmax, 513 of F) and a two-block factor"""
    _check_fused(gpu_ctx, LARGE, ("matern52",), "fused large")
