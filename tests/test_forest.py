"""The regression forest: the presort, the grow kernel and the tree sweep (robo_amd/csrc/forest.hip, api_forest.hip) and
models/forest.py against the replay of tests/forest_oracle.py, whose docstring derives the bounds.  CPU: through the
interpreter (tests/hipemu).  -m gpu: the same checks on the MI355X.
Largest error / bound observed: NOTES.md "Random forest".
"""
import os
import pickle
import sys

import numpy as np
import pytest

from robo_amd import _lib
from robo_amd.acquisition_functions import EI
from robo_amd.models import RandomForest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_oracle as FO  # noqa: E402
from _tol import ACQ_RTOL  # noqa: E402
from test_ehvi import _bits, emu_ctx, gpu_ctx  # noqa: E402,F401

EPS, SEED = FO.EPS, 0x1234567887654321
# n, D, T, bootstrap, max_features, data, options
CASES = [(1, 1, 1, False, 1, "rand", {}), (2, 3, 1, True, 3, "rand", {}), (3, 3, 30, True, 1, "rand", {}),
         (63, 1, 1, False, 1, "rand", {}), (64, 3, 1, True, 3, "dups", {}), (65, 64, 1, True, 5, "rand", {}),
         (64, 64, 1, False, 64, "rand", {}), (65, 3, 30, True, 1, "rand", {}), (255, 3, 1, False, 3, "consty", {}),
         (256, 3, 2, True, 1, "dups", {}), (257, 3, 1, True, 3, "constcol", {}), (513, 1, 1, True, 1, "rand", {}),
         (1000, 3, 1, False, 3, "rand", {}),
         (257, 3, 1, False, 2, "rand", dict(min_samples_split=8, min_samples_leaf=3, max_depth=4, eps_purity=1e-3))]


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def ctx(request):
    return request.getfixturevalue(request.param + "_ctx")


def _data(n, D, kind):
    rs = np.random.RandomState(n + D)
    X = rs.randint(0, 3, (n, D)) * 0.5 - 0.5 if kind == "dups" else rs.rand(n, D) * 2.0 - 0.6
    if kind == "constcol":
        X[:, 0] = 0.25
    y = np.full(n, 3.5) if kind == "consty" else np.sin(3 * X[:, 0]) + X[:, -1] ** 2 + 0.1 * rs.randn(n) + 5.0
    return X, y


def _forest(ctx, n, D, T, boot, mf, kind, opts, idx=None, total_variance=True):
    X, y = _data(n, D, kind)
    rf = _lib.DeviceForest(ctx, D, T, boot, mf, total_variance=total_variance, **opts)
    rf.fit(X, y, seed=SEED, idx=idx)
    return rf, X, y


def _check_growth(rf, X, y, T, boot, mf, opts, idx=None):
    worst = 0.0
    for t, tree in enumerate(rf.trees):
        w = FO.weights(SEED, t, len(y), len(y), idx) if boot else np.ones(len(y), dtype=np.int64)
        worst = max(worst, FO.replay(tree, X, y, w, t, SEED, mf, **opts))
    print("growth error / bound %.3g" % worst)
    assert worst <= 1.0


@pytest.mark.parametrize("n,D,T,boot,mf,kind,opts", CASES)
def test_growth(ctx, n, D, T, boot, mf, kind, opts):
    rf, X, y = _forest(ctx, n, D, T, boot, mf, kind, opts)
    _check_growth(rf, X, y, T, boot, mf, opts)
    if n == 1 or kind == "consty":
        assert all(len(tr) == 1 for tr in rf.trees)            # the root is a leaf
    rf.close()


def test_growth_given_draws(ctx):
    """the caller's table: tree 0 draws one row n times (its root is a leaf), tree 1 the rows Philox would have drawn"""
    n, D = 65, 3
    idx = np.stack([np.full(n, 7), np.minimum((FO.BO.philox(np.arange(n), 0, 1, 0x52460000, SEED)[0] * float(n)).astype(np.int64), n - 1)])
    rf, X, y = _forest(ctx, n, D, 2, True, 3, "rand", {}, idx=idx)
    _check_growth(rf, X, y, 2, True, 3, {}, idx=idx)
    own, _, _ = _forest(ctx, n, D, 2, True, 3, "rand", {})
    assert len(rf.trees[0]) == 1 and rf.trees[0]["mean"][0] == y[7] and rf.trees[1].tobytes() == own.trees[1].tobytes()
    rf.close(), own.close()


def test_independence(ctx):
    """tree t has the same bits whatever the number of trees, and across two fits with one seed"""
    ref, X, y = _forest(ctx, 65, 3, 30, True, 1, "rand", {})
    trees = ref.trees
    for T in (1, 7):
        rf, _, _ = _forest(ctx, 65, 3, T, True, 1, "rand", {})
        assert all(a.tobytes() == b.tobytes() for a, b in zip(rf.trees, trees)), T
        rf.close()
    ref.fit(X, y, seed=SEED)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ref.trees, trees))
    ref.fit(X, y, seed=SEED + 1)
    assert any(a.tobytes() != b.tobytes() for a, b in zip(ref.trees, trees))
    ref.close()


@pytest.mark.parametrize("n,D,T,boot,total", [(63, 3, 30, True, True), (1000, 3, 2, False, True), (65, 64, 3, True, False),
                                              (64, 1, 1, False, True)])
def test_sweep(ctx, n, D, T, boot, total):
    """n = 1000 without bootstrapping: 1999 nodes a tree, read through L2; the others are walked in LDS"""
    rf, X, y = _forest(ctx, n, D, T, boot, D, "rand", {}, total_variance=total)
    trees = rf.trees
    assert (max(len(tr) for tr in trees) > _lib.RF_STAGE_NODES) == (n == 1000)
    rs = np.random.RandomState(n)
    Xc = np.concatenate((X[:50], rs.rand(4099 - 50, D) * 2.4 - 0.8))
    mean, var, pt = rf.predict(Xc, per_tree=True)
    mu, v = FO.walk(trees, Xc)
    mo, vo, E, dv = FO.moments(mu, v, total)
    print("sweep error / bound: mean %.3g var %.3g" % (np.max(np.abs(mean - mo) / E), np.max(np.abs(var - np.maximum(vo, EPS)) / (dv + EPS * EPS))))
    assert _bits(pt, mu) and np.all(np.abs(mean - mo) <= E) and np.all(np.abs(var - np.maximum(vo, EPS)) <= dv) and np.all(var >= EPS)
    for m in (1, 255, 257):                                       # other batch sizes and positions: the same bits
        assert all(_bits(u, w[:m]) for u, w in zip(rf.predict(Xc[:m]), (mean, var))), m
    back = rf.predict(np.concatenate((Xc[:3], Xc[:300][::-1])))
    assert _bits(back[0][3:][::-1], mean[:300]) and _bits(back[1][3:][::-1], var[:300])
    bad = rf.predict(np.where(np.arange(D) == D - 1, np.nan, Xc[:2]), per_tree=True)
    assert all(np.all(np.isnan(b)) for b in bad)
    for acq, par in (("ei", 0.0), ("log_ei", 0.01), ("pi", 0.0), ("lcb", 2.0)):
        vals, mx, am, fl = rf.acq(acq, par, float(y.min()), Xc)
        want = _lib.acq_from_moments(ctx, acq, par, float(y.min()), mean, var)
        assert np.allclose(vals, want[0], rtol=ACQ_RTOL, atol=0) and np.isclose(mx, want[1], rtol=ACQ_RTOL, atol=0)
        assert (am, fl) == want[2:] and rf.acq(acq, par, float(y.min()), Xc, want_values=False)[1:] == (mx, am, fl), acq
    rf.close()


def test_refusals(ctx):
    for bad in (dict(dim=0), dict(dim=65), dict(n_trees=0), dict(n_trees=129), dict(max_features=0), dict(max_features=3),
                dict(min_samples_split=0), dict(min_samples_leaf=0), dict(max_depth=-1), dict(eps_purity=-1.0), dict(eps_purity=np.nan)):
        with pytest.raises(ValueError):
            _lib.DeviceForest(ctx, **dict(dict(dim=2, n_trees=2), **bad))
    rf, X, y = _lib.DeviceForest(ctx, 2, 2), np.random.RandomState(0).rand(9, 2), np.arange(9.0)
    for call in (lambda: rf.predict(X), lambda: rf.acq("ei", 0.0, 0.0, X), lambda: rf.trees):
        with pytest.raises(Exception, match="trained first"):
            call()
    for call in (lambda: rf.fit(X[:0], y[:0]), lambda: rf.fit(np.zeros((4097, 2)), np.zeros(4097)), lambda: rf.fit(X, y, n_points=-1),
                 lambda: rf.fit(X, np.where(np.arange(9) == 4, np.nan, y)), lambda: rf.fit(np.where(X > 0.9, np.inf, X), y),
                 lambda: rf.fit(X, y, idx=np.full((2, 9), 9)), lambda: rf.fit(X, y, idx=np.full((2, 9), -1))):
        with pytest.raises(ValueError):
            call()
    rf.fit(X, y)
    trees = rf.trees
    for field, value in (("feature", 2), ("left", 0), ("right", 99), ("threshold", np.nan)):
        broken = [tr.copy() for tr in trees]
        broken[1][field][0] = value
        with pytest.raises(ValueError):
            rf.set_trees(broken)
    with pytest.raises(ValueError):
        rf.predict(X[:0])
    so = _lib.lib()                                              # every NULL required pointer; destroy(NULL) is harmless
    for status in (so.robo_rf_fit(rf._h, None, None, 9, 9, 0, None), so.robo_rf_get_trees(rf._h, None, None, None),
                   so.robo_rf_set_trees(rf._h, None, 1, None), so.robo_rf_predict(rf._h, None, 9, None, None, None),
                   so.robo_rf_create(ctx._h, 2, 2, 1, 2, 2, 1, 8, 0.0, 1, None)):
        assert status == _lib.BAD_ARGUMENT
    assert so.robo_rf_destroy(None) == 0
    rf.close()


def test_class(ctx, monkeypatch):
    """RandomForest on a seeded toy: the fused path of EI equals the moments path, a pickle predicts the same bits, the
    solver calls the objective once per iteration"""
    from robo_amd.maximizers import RandomSampling
    from robo_amd.solver.bayesian_optimization import BayesianOptimization
    X, y = _data(40, 2, "rand")
    model = RandomForest(rng=np.random.RandomState(1), ctx=ctx)
    assert (model.num_trees, model.do_bootstrapping, model.n_points_per_tree, model.compute_oob_error) == (30, True, 0, False)
    with pytest.raises(Exception, match="trained first"):
        model.predict(X)
    for bad in (dict(num_trees=0), dict(min_samples_leaf=0), dict(max_features=0), dict(eps_purity=-1.0)):
        with pytest.raises(ValueError):
            RandomForest(**bad)
    model.train(X, y)
    Xt = np.random.RandomState(2).rand(65, 2) * 2.0 - 0.6
    mean, var = model.predict(Xt)
    each = model.predict_each_tree(Xt)
    assert each.shape == (30, 65) and np.allclose(each.mean(axis=0), mean, rtol=1e-13) and model.get_incumbent()[1] == y.min()
    twin = pickle.loads(pickle.dumps(model))
    twin._ctx = ctx
    assert all(_bits(a, b) for a, b in zip(twin.predict(Xt), (mean, var)))
    want = _lib.acq_from_moments(ctx, "ei", 0.0, float(y.min()), mean, var)
    monkeypatch.setattr(model, "predict", None)                   # EI answers from the fused call alone
    acq = EI(model)
    assert np.allclose(np.ravel(acq.compute(Xt)), want[0], rtol=ACQ_RTOL, atol=0) and acq.argmax(Xt) == want[2]
    with pytest.raises(ImportError):
        import robo_amd.models.random_forest  # noqa: F401

    calls, lower, upper = [], np.array([-5.0, 0.0]), np.array([10.0, 15.0])

    def branin(x):
        calls.append(x)
        return (x[1] - 5.1 / (4 * np.pi ** 2) * x[0] ** 2 + 5 / np.pi * x[0] - 6) ** 2 + 10 * (1 - 1 / (8 * np.pi)) * np.cos(x[0]) + 10

    rng = np.random.RandomState(5)
    model = RandomForest(num_trees=5, rng=rng, ctx=ctx)
    acq = EI(model)
    bo = BayesianOptimization(branin, lower, upper, acq, model, RandomSampling(acq, lower, upper, rng=rng, n_samples=200),
                              initial_points=3, rng=rng)
    inc, val = bo.run(8)
    assert len(calls) == 8 and np.isfinite(val) and np.shape(inc) == (2,)
