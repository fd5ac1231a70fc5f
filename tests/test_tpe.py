"""Parzen estimators and TPE: the prepare and sweep kernels (robo_amd/csrc/kde.hip, api_kde.hip), models/tpe.py, DensityRatio,
ParzenSampling and the front end against tests/tpe_oracle.py, whose docstring derives the bounds.  CPU: through the interpreter
(tests/hipemu).  -m gpu: the same checks on the MI355X.  Largest error / bound observed: NOTES.md "Parzen estimators".
"""
import os
import sys

import numpy as np
import pytest

from robo_amd import _lib
from robo_amd.models import tpe as T

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tpe_oracle as O  # noqa: E402
from test_ehvi import _bits, emu_ctx, gpu_ctx  # noqa: E402,F401


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def ctx(request):
    return request.getfixturevalue(request.param + "_ctx")


def _mixture(rs, lo, hi, n, shared, weights, h_scale=0.3):
    D = lo.shape[0]
    mu = lo + (hi - lo) * rs.rand(n, D)
    h = (hi - lo) * h_scale * (0.05 + rs.rand(*((D,) if shared else (n, D))))
    return mu, h, (0.1 + rs.rand(n)) if weights else None


def _kde(ctx, n, D, shared, weights, seed=0, **how):
    rs = np.random.RandomState(1000 * n + D + seed)
    lo = -1.0 - rs.rand(D)
    hi = lo + 0.5 + 2.0 * rs.rand(D)
    kde = _lib.DeviceKDE(ctx, lo, hi)
    mixes = [_mixture(rs, lo, hi, n, shared, weights, **how), _mixture(rs, lo, hi, n + 3, not shared, weights, **how)]
    for which, mix in enumerate(mixes):
        kde.set_mixture(which, *mix)
    return kde, lo, hi, mixes, rs


def _check(kde, lo, hi, mixes, X, tag):
    """the terms against the formulas, the sweep against the device's own terms -> the fused call's result"""
    res = kde.ratio(X)
    worst = 0.0
    for which, mix in enumerate(mixes):
        c, psi = kde.terms(which)
        oc, opsi, bc, bpsi = O.terms(lo, hi, *mix)
        fin = np.isfinite(oc)
        assert np.all(c[~fin] == -np.inf) and np.all(np.abs(c[fin] - oc[fin]) <= bc[fin]) and np.all(np.abs(psi - opsi) <= bpsi), tag
        lp, bound = O.sweep(lo, hi, c, psi, X)
        ok = ~np.isnan(lp)
        assert np.all(np.isfinite(res[1 + which][ok])) and np.all(np.isnan(res[1 + which][~ok])), tag
        worst = max(worst, float(np.max(np.abs(c[fin] - oc[fin]) / bc[fin])), float(np.max(np.abs(res[1 + which][ok] - lp[ok]) / bound[ok])))
    print("%s: error / bound %.3g" % (tag, worst))
    assert worst <= 1.0, tag
    assert _bits(res[0], res[1] - res[2]) and res[4] == int(np.argmax(res[0])) and _bits(res[3], res[0][res[4]]), tag
    return res


# n: 1, below / at / above one 16-component block, three blocks, one more than a staging chunk; m: 1, around a wave's 16
# candidates, one more than a tile; D: 2 D below, at and off a multiple of 4, and the widest
@pytest.mark.parametrize("n,m,D,shared,weights", [(1, 1, 1, True, False), (15, 15, 2, False, True), (16, 16, 3, True, True),
                                                  (17, 17, 17, False, False), (33, 65, 64, True, True),
                                                  (_lib.KDE_CHUNK + 1, 65, 3, False, True), (17, 65, 16, True, False)])
def test_sweep(ctx, n, m, D, shared, weights):
    kde, lo, hi, mixes, rs = _kde(ctx, n, D, shared, weights)
    X = lo + (hi - lo) * rs.rand(m, D)
    res = _check(kde, lo, hi, mixes, X, "n %d m %d D %d" % (n, m, D))
    assert res[5] == 0
    kde.close()


def test_sweep_edges(ctx):
    # h = 1e-3 of the width and a candidate 0.9 away: every exponent is near -4e5
    kde, lo, hi, mixes, rs = _kde(ctx, 17, 2, True, False, h_scale=1e-3 / 0.55)
    mu = lo + (hi - lo) * 0.05 * rs.rand(17, 2)
    for which in (0, 1):
        mixes[which] = (mu, mixes[0][1], None)
        kde.set_mixture(which, *mixes[which])
    res = _check(kde, lo, hi, mixes, mu[:5] + 0.9 * (hi - lo), "narrow")
    assert np.all(res[1] < -1e5)
    kde.close()
    # the first 16 components weigh nothing: whatever they are, the same bits, and never NaN
    kde, lo, hi, mixes, rs = _kde(ctx, 33, 3, False, True)
    w = np.where(np.arange(33) < 16, 0.0, mixes[0][2])
    mixes[0] = (mixes[0][0], mixes[0][1], w)
    kde.set_mixture(0, *mixes[0])
    X = lo + (hi - lo) * rs.rand(20, 3)
    res = _check(kde, lo, hi, mixes, X, "zero weights")
    other = _mixture(rs, lo, hi, 33, False, True)
    kde.set_mixture(0, np.where(np.arange(33)[:, None] < 16, other[0], mixes[0][0]), np.where(np.arange(33)[:, None] < 16, other[1], mixes[0][1]), w)
    assert all(_bits(a, b) for a, b in zip(kde.ratio(X)[:3], res[:3])) and not np.any(np.isnan(res[0]))
    # a NaN coordinate: NaN in all three, the flag, the argmax on that row
    X[7, 2] = np.nan
    res = kde.ratio(X)
    assert all(np.isnan(v[7]) and not np.any(np.isnan(np.delete(v, 7))) for v in res[:3])
    assert res[4] == 7 and np.isnan(res[3]) and res[5] == _lib.FLAG_NAN and kde.ratio(X[:7])[5] == 0
    kde.close()


def test_invariance(ctx):
    D = 5
    kde, lo, hi, mixes, rs = _kde(ctx, 40, D, False, True)
    X = lo + (hi - lo) * rs.rand(300, D)
    ref = kde.ratio(X)
    alone = kde.ratio(X[:1])
    Xb = X[100:165].copy()
    Xb[[0, 16, 63]] = X[0]
    moved = kde.ratio(Xb)
    assert all(_bits(moved[i][[0, 16, 63]], np.repeat(alone[i], 3)) and _bits(alone[i], ref[i][:1]) for i in range(3))
    ctx.set_tuning("ws_bytes", 128 * D * 8)               # a one-block workspace: three passes
    try:
        passes = kde.ratio(X)
    finally:
        ctx.set_tuning("ws_bytes", None)
    assert all(_bits(a, b) for a, b in zip(passes[:4], ref[:4])) and passes[4:] == ref[4:]
    assert _bits(kde.logpdf(0, X), ref[1]) and _bits(kde.logpdf(1, X), ref[2]) and kde.ratio(X, want_values=False)[3:] == ref[3:]
    kde.close()


_BOX = (np.zeros(2), np.ones(2))
_MU, _H = np.full((3, 2), 0.5), np.full((3, 2), 0.1)


@pytest.mark.parametrize("bad", [lambda c: _lib.DeviceKDE(c, np.zeros(0), np.zeros(0)), lambda c: _lib.DeviceKDE(c, np.zeros(65), np.ones(65)),
                                 lambda c: _lib.DeviceKDE(c, np.ones(2), np.ones(2)), lambda c: _lib.DeviceKDE(c, [0.0, -np.inf], [1.0, 1.0]),
                                 lambda c: _lib.DeviceKDE(c, [0.0, 0.0], [1.0, np.nan]),
                                 lambda k: k.set_mixture(0, np.full((3, 2), 1.5), _H), lambda k: k.set_mixture(0, _MU * np.nan, _H),
                                 lambda k: k.set_mixture(0, _MU, _H * 0.0), lambda k: k.set_mixture(0, _MU, -_H[0]),
                                 lambda k: k.set_mixture(0, _MU, _H * np.inf), lambda k: k.set_mixture(0, _MU, _H, [1.0, -1.0, 1.0]),
                                 lambda k: k.set_mixture(0, _MU, _H, [1.0, np.inf, 1.0]), lambda k: k.set_mixture(0, _MU, _H, np.zeros(3)),
                                 lambda k: k.set_mixture(2, _MU, _H), lambda k: k.set_mixture(0, _MU[:0], _H[:0]),
                                 lambda k: k.ratio(_MU[:0]), lambda k: k.logpdf(0, _MU[:0])])
def test_refusals(ctx, bad):
    kde = _lib.DeviceKDE(ctx, *_BOX)
    for call in (lambda: kde.ratio(_MU), lambda: kde.logpdf(1, _MU), lambda: kde.terms(0)):
        with pytest.raises(Exception, match="trained first"):
            call()
    kde.set_mixture(0, _MU, _H)
    with pytest.raises(Exception, match="trained first"):
        kde.ratio(_MU)                                      # the bad mixture is still missing
    kde.set_mixture(1, _MU, _H[0])
    with pytest.raises(ValueError):
        bad(ctx if bad.__code__.co_varnames[0] == "c" else kde)
    so, p, out = _lib.lib(), _lib._arr(_MU), np.empty(3)    # every NULL required pointer, n out of range; destroy(NULL) is harmless
    for status in (so.robo_kde_create(ctx._h, 2, None, p, None), so.robo_kde_set_mixture(kde._h, 0, None, p, 0, None, 3),
                   so.robo_kde_set_mixture(kde._h, 0, p, p, 0, None, (1 << 20) + 1), so.robo_kde_get_terms(kde._h, 0, None, None),
                   so.robo_kde_logpdf(kde._h, 0, p, 3, None), so.robo_kde_ratio_eval_cand(kde._h, p, 3, None, None, None, None, None, None),
                   so.robo_kde_ratio_eval_cand(kde._h, None, 3, None, None, None, _lib._arr(out), None, None)):
        assert status == _lib.BAD_ARGUMENT
    assert so.robo_kde_destroy(None) == 0 and np.all(np.isfinite(kde.ratio(_MU)[0]))       # the handle stays usable
    kde.close()


def test_host_rules():
    """the split, both bandwidth rules and the draws from l(x), in NumPy alone"""
    good, bad = T.split(np.array([3.0, 1.0, 1.0, 0.5, 1.0, 2.0, 1.0]), 0.15)          # n = 7: ceil(1.05) = 2; ties keep their order
    assert good.tolist() == [3, 1] and bad.tolist() == [2, 4, 6, 5, 0]
    assert [len(T.split(np.arange(n)[::-1], 0.15)[0]) for n in (2, 7, 100)] == [1, 2, 15] and len(T.split(np.zeros(2), 0.9)[0]) == 1
    # sorted with the prior's 0.5: 0.1, 0.2, 0.5, 0.9 -> gaps 0.1, 0.3, 0.4; the clip is [1 / 4, 1]
    mu, h, w = T.hyperopt_mixture(np.array([[0.2], [0.9], [0.1]]), prior_weight=2.0)
    assert mu.ravel().tolist() == [0.2, 0.9, 0.1, 0.5] and w.tolist() == [1.0, 1.0, 1.0, 2.0]
    assert np.allclose(h.ravel(), [0.3, 0.4, 0.25, 1.0], rtol=1e-15)
    mu, h, w = T.scott_mixture(np.array([[0.0, 0.3], [1.0, 0.3]]), 1e-3)
    assert w is None and np.allclose(h, [1.06 * 0.5 * 2 ** (-1 / 6.0), 1e-3], rtol=1e-15)
    model = T.TPE(np.array([-5.0, 0.0]), np.array([10.0, 15.0]), rng=np.random.RandomState(0))
    model._dev, model.mixtures = object(), [(np.array([[0.2, 1.0], [0.9, 0.0]]), np.array([[0.5, 2.0], [1e-9, 1e-9]]), np.array([1.0, 0.0])), None]
    draws = model.sample_good(500)
    assert draws.shape == (500, 2) and np.all(draws >= model.lower) and np.all(draws <= model.upper) and draws[:, 1].std() > 1.0
    model.mixtures[0] = model.mixtures[0][:2] + (np.array([0.0, 1.0]),)              # the narrow component alone
    assert np.allclose(model.sample_good(50), [8.5, 0.0], atol=1e-6)
    with pytest.raises(NotImplementedError, match="ratio"):
        model.predict(np.zeros((1, 2)))


@pytest.mark.parametrize("maximizer", ["random", "parzen"])
def test_front_end(emu_ctx, monkeypatch, maximizer):
    """five iterations on Branin: every proposal is the oracle's argmax over its candidates, or tied with it within the bound"""
    from robo_amd.acquisition_functions import DensityRatio
    from robo_amd.fmin import bayesian_optimization
    lower, upper, seen = np.array([-5.0, 0.0]), np.array([10.0, 15.0]), []
    argmax = DensityRatio.argmax
    monkeypatch.setattr(DensityRatio, "argmax", lambda self, X: seen.append((X, argmax(self, X))) or seen[-1][1])

    def branin(x):
        return (x[1] - 5.1 / (4 * np.pi ** 2) * x[0] ** 2 + 5 / np.pi * x[0] - 6) ** 2 + 10 * (1 - 1 / (8 * np.pi)) * np.cos(x[0]) + 10

    np.random.seed(3)
    res = bayesian_optimization(branin, lower, upper, num_iterations=8, n_init=3, model_type="tpe", acquisition_func="ei",
                                maximizer=maximizer, n_candidates=40, rng=np.random.RandomState(3))
    Xs, ys = np.array(res["X"]), np.array(res["y"])
    assert len(seen) == 5 and Xs.shape == (8, 2)
    for it, (cand, pick) in enumerate(seen):
        Z = (Xs[:3 + it] - lower) / (upper - lower)
        mixes = [T.hyperopt_mixture(Z[idx]) for idx in T.split(ys[:3 + it], 0.15)]
        zc = (cand - lower) / (upper - lower)
        want = O.logpdf(0, 1, *mixes[0], zc) - O.logpdf(0, 1, *mixes[1], zc)
        tol = sum(float(np.max(O.terms(np.zeros(2), np.ones(2), *mx)[2]) + np.max(O.sweep(np.zeros(2), np.ones(2), *[t.astype(np.float64) for t in O.terms(np.zeros(2), np.ones(2), *mx)[:2]], zc)[1])) for mx in mixes)
        assert want[pick] >= want.max() - 2 * tol and np.array_equal(Xs[3 + it], cand[pick]), it
    for bad in (dict(acquisition_func="pi"), dict(maximizer="scipy"), dict(batch_size=2)):
        with pytest.raises(ValueError):
            bayesian_optimization(lambda x: pytest.fail("the objective was called"), lower, upper, num_iterations=8,
                                  **dict(dict(model_type="tpe", acquisition_func="ei", maximizer="random"), **bad))


@pytest.mark.gpu
def test_sweep_at_size(gpu_ctx):
    """n = 4096 and the prior, D = 16, a batch that ends inside a tile"""
    rs, D, m = np.random.RandomState(9), 16, 32773
    kde = _lib.DeviceKDE(gpu_ctx, np.zeros(D), np.ones(D))
    mixes = [T.hyperopt_mixture(rs.rand(4096, D)), T.hyperopt_mixture(0.2 + 0.6 * rs.rand(1024, D))]
    for which, mix in enumerate(mixes):
        kde.set_mixture(which, *mix)
    X = rs.rand(m, D)
    res = kde.ratio(X)
    sub = np.arange(0, m, m // 512 + 1)
    worst = 0.0
    for which in (0, 1):
        lp, bound = O.sweep(np.zeros(D), np.ones(D), *kde.terms(which), X[sub])
        worst = max(worst, float(np.max(np.abs(res[1 + which][sub] - lp) / bound)))
    print("at size: error / bound %.3g" % worst)
    assert worst <= 1.0 and res[4] == int(np.argmax(res[0])) and _bits(res[0], res[1] - res[2]) and res[5] == 0
    kde.close()
