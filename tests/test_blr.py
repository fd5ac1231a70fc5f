"""Bayesian linear regression on basis features (robo_amd/csrc/blr.hip, api_blr.hip, models/bayesian_linear_regression.py)
against the plain long-double oracle of tests/blr_oracle.py.  CPU: through the interpreter (tests/hipemu).  -m gpu: the same
checks on the MI355X, plus N = 2^18, F = 128 random Fourier features with a fused sweep over 65 536 candidates.
Bounds.  Statistics: derived, (chunk accumulation length + chunks) eps sum_i |phi_if phi_ig| (+ the cosine's and its argument's
rounding for kind 3).  The other constants are 4 x the largest error / unit observed, rounded up (NOTES.md):
  eigenpairs   max(residual / (F eps |G|_F), orthogonality / (F eps)): interpreter 1.69, MI355X 1.35 -> C_EIG = 7
  likelihood   error / (F eps (|mll| + beta yy)):                     below 0.25 on both                -> C_LL = 1
  sweep        error / (F eps sum_j |psi_j c_j| beta / t_j), the variance likewise: below 2.6 on both   -> C_SWEEP = 11
Two nearly singular cases carry constants of their own in their parameter lists (128 random Fourier features of 300 rows:
likelihood, interpreter 607, MI355X 239 -> 2500; 17 random Fourier features of a one-dimensional input: sweep, interpreter
1930, MI355X 5799 -> 24000): there the rounding of G itself, eps |G| beta against t_min = alpha, moves the posterior, and any
fp64 Phi^T Phi differs from the long-double oracle by as much.
"""
import os
import sys

import numpy as np
import pytest

from robo_amd import _lib
from robo_amd.acquisition_functions import EI, LCB, PI, LogEI
from robo_amd.models.bayesian_linear_regression import (BayesianLinearRegression, RandomFourierBasis, linear_basis_func,
                                                        quadratic_basis_func)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blr_oracle as O  # noqa: E402
from golden.make_golden_blr import THETAS, inputs  # noqa: E402
from oracle import gp_oracle  # noqa: E402
from test_ehvi import _bits, emu_ctx, gpu_ctx  # noqa: E402,F401

LD, EPS, C, T = O.LD, O.EPS, _lib.BLR_CHUNK, _lib.BLR_TILE
C_EIG, C_LL, C_SWEEP = 7, 1, 11
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_blr.npz")


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def ctx(request):
    return request.getfixturevalue(request.param + "_ctx")


def _model(ctx, kind, D, F, N, seed=0, dup=False):
    """a handle with data -> handle, rows, y, the oracle's Phi, the feature arguments"""
    rs = np.random.RandomState(seed + 7 * F + N)
    feat = dict(omega=rs.randn(D, F) * 2.0, phase=rs.rand(F) * 2 * np.pi, scale=np.sqrt(2.0 / F)) if kind == "rff" else {}
    X = rs.rand(N, F if kind == "given" else D) * 2.0 - 0.6
    if dup:
        X[:, -1] = X[:, 0]
    y = np.sin(3 * X[:, 0]) + X[:, -1] ** 2 + 0.1 * rs.randn(N)
    h = _lib.DeviceBLR(ctx, kind, D, F, **feat)
    h.set_data(X, y)
    return h, X, y, O.features(kind, X, **feat), feat


@pytest.mark.parametrize("kind,D,F,N", [
    ("given", 1, 1, 1), ("given", 1, 15, C - 1), ("given", 1, 128, C + 1), ("linear", 1, 2, C), ("linear", 17, 18, 2 * C + 5),
    ("quadratic", 3, 7, C + 1), ("quadratic", 17, 35, C - 1), ("rff", 1, 16, 2 * C + 5), ("rff", 3, 17, 1), ("rff", 17, 128, C),
    ("rff", 3, 15, C + 1)])
def test_stats(ctx, kind, D, F, N):
    h, X, y, Phi, feat = _model(ctx, kind, D, F, N)
    G, b, yy, _, _ = h.stats()
    c = (min(N, C) + (N + C - 1) // C) * EPS
    A, yl = np.abs(Phi), np.asarray(y, dtype=LD)
    bound_G, bound_b = c * (A.T @ A), c * (A.T @ np.abs(yl))
    if kind == "rff":        # d phi <= scale (2 eps + (D + 2) eps (|x| . |omega| + |phase|)): the cosine, then its argument
        dphi = feat["scale"] * EPS * (2 + (D + 2) * (O.rff_argument(X, feat["omega"]) + np.abs(feat["phase"])))
        bound_G = bound_G + dphi.T @ A + A.T @ dphi
        bound_b = bound_b + dphi.T @ np.abs(yl)
    assert np.all(np.abs(G - Phi.T @ Phi) <= bound_G) and np.all(np.abs(b - Phi.T @ yl) <= bound_b)
    assert abs(yy - yl @ yl) <= c * (yl @ yl) and _bits(G, G.T)
    h.set_data(X, y)                                             # a second call; then one chunk's partial at a time
    assert all(_bits(u, v) for u, v in zip(h.stats(), (G, b, yy)))
    ctx.set_tuning("ws_bytes", 8)
    try:
        h.set_data(X, y)
    finally:
        ctx.set_tuning("ws_bytes", None)
    assert all(_bits(u, v) for u, v in zip(h.stats(), (G, b, yy)))
    for bad in (np.nan, np.inf):                                 # a non-finite row or target is refused, not factored
        Xb, yb = X.copy(), y.copy()
        Xb[N // 2, 0] = bad
        yb[N - 1] = -bad
        for rows, targets in ((Xb, y), (X, yb)):
            with pytest.raises(ValueError):
                h.set_data(rows, targets)
    h.close()


@pytest.mark.parametrize("F,N,dup", [(1, 5, False), (2, 9, False), (17, 40, False), (128, 300, False), (17, 5, False),
                                     (17, 40, True)])
def test_eig(ctx, F, N, dup):
    h, X, y, Phi, _ = _model(ctx, "given", 1, F, N, dup=dup)
    G, b, yy, lam, Q = (np.asarray(a, dtype=LD) for a in h.stats())
    res = np.abs(G @ Q - Q * lam).max() / (F * EPS * max(np.sqrt((G * G).sum()), LD(1e-300)))
    assert res <= C_EIG and np.abs(Q.T @ Q - np.eye(F)).max() / (F * EPS) <= C_EIG
    th = np.stack((np.linspace(-12, 2, 7), np.linspace(14, -2, 7)), axis=1)
    assert np.all(lam >= 0) and np.all(np.isfinite(h.loglik(th, 0))) and np.all(np.isfinite(h.loglik(th, 1)))
    if N < F or dup:
        assert np.sum(np.asarray(lam, dtype=np.float64) <= 1e-12 * float(lam.max())) >= (1 if dup else F - N)
    h.close()


@pytest.mark.parametrize("kind,D,F,N,S,limit", [("linear", 3, 4, 60, 1, C_LL), ("quadratic", 17, 35, 200, 20, C_LL),
                                                ("rff", 3, 128, 300, 20, 2500), ("given", 1, 17, 80, 64, C_LL)])
def test_loglik(ctx, kind, D, F, N, S, limit):
    h, X, y, Phi, _ = _model(ctx, kind, D, F, N, seed=S)
    rs = np.random.RandomState(S)
    th = np.stack((rs.uniform(-12, 2, S), rs.uniform(-2, 14, S)), axis=1)
    yy = float(y @ y)
    for form in (0, 1):
        ll = h.loglik(th, form)
        assert _bits(ll, np.concatenate([h.loglik(t[None], form) for t in th]))
        for s, (la, lb) in enumerate(th):
            ref = O.Posterior(Phi, y, np.exp(LD(la)), np.exp(LD(lb))).loglik(form)
            assert abs(LD(ll[s]) - ref) <= limit * F * EPS * (abs(ref) + np.exp(lb) * yy), (form, s)
    h.close()


@pytest.mark.parametrize("kind,D,F,S,limit", [
    ("given", 1, 1, 1, C_SWEEP), ("given", 1, 15, 20, C_SWEEP), ("linear", 3, 4, 64, C_SWEEP), ("quadratic", 17, 35, 20, C_SWEEP),
    ("rff", 3, 16, 1, C_SWEEP), ("rff", 1, 17, 64, 24000), ("rff", 17, 128, 20, C_SWEEP), ("given", 1, 128, 1, C_SWEEP)])
def test_sweep(ctx, kind, D, F, S, limit):
    h, X, y, Phi, feat = _model(ctx, kind, D, F, 150, seed=S)
    rs = np.random.RandomState(F + S)
    ab = np.exp(np.stack((rs.uniform(-4, 2, S), rs.uniform(0, 8, S)), axis=1))
    with pytest.raises(Exception, match="trained first"):
        h.predict(X)                                             # data, no hyper-parameter samples yet
    h.set_hypers(ab)
    Xc = rs.rand(401, X.shape[1]) * 2.0 - 0.6
    mean, var, pm, pv = h.predict(Xc, per_sample=True)
    _, b, _, lam, Q = (np.asarray(a, dtype=LD) for a in h.stats())
    phi = O.features(kind, Xc, **feat)
    psi, c = np.abs(phi @ Q), np.abs(Q.T @ b)
    for s, (alpha, beta) in enumerate(ab):
        mo, vo = O.Posterior(Phi, y, alpha, beta).predict(phi)
        t = beta * lam + alpha
        assert np.all(np.abs(pm[s] - mo) <= limit * F * EPS * np.maximum((psi * c * beta / t).sum(axis=1), LD(1e-300))), s
        assert np.all(np.abs(pv[s] - vo) <= limit * F * EPS * (1 / beta + (psi * psi / t).sum(axis=1))), s
    mix_m, mix_v = O.mixture(pm.astype(LD), pv.astype(LD))
    assert np.all(np.abs(mean - mix_m) <= 4 * EPS * np.abs(pm).mean(axis=0)) and np.all(np.abs(var - mix_v) <= 4 * EPS * mix_v)
    for m in (1, T - 1, T, T + 1):                               # other batch sizes and positions: the same bits
        sub = h.predict(Xc[:m])
        assert _bits(sub[0], mean[:m]) and _bits(sub[1], var[:m]), m
    back = h.predict(np.concatenate((Xc[:3], Xc[::-1])))
    assert _bits(back[0][3:][::-1], mean) and _bits(back[1][3:][::-1], var)
    bad = Xc[:T + 2].copy()
    bad[T, 0] = np.nan
    got = h.predict(bad)
    assert np.isnan(got[0][T]) and np.isnan(got[1][T]) and _bits(np.delete(got[0], T), np.delete(mean[:T + 2], T))
    h.set_hypers(np.full((S, 2), 1e30))                          # the eps clip
    assert _bits(h.predict(Xc[:5])[1], np.full(5, EPS))
    h.close()


def _check_fused(ctx, kind, D, F, m):
    h, X, y, _, _ = _model(ctx, kind, D, F, 90)
    h.set_hypers(np.array([[1.0, 1000.0], [0.1, 50.0], [3.0, 400.0]]))
    Xc = np.random.RandomState(m).rand(m, X.shape[1]) * 2.0 - 0.6
    for acq, par in (("ei", 0.0), ("log_ei", 0.01), ("pi", 0.0), ("lcb", 2.0)) if m < 1000 else (("ei", 0.0),):
        for edit in ((), ((m // 2, m // 3),), ((m - 1, None),)):  # plain, a tie, a NaN row
            Xe = Xc.copy()
            for dst, src in edit:
                Xe[dst] = np.nan if src is None else Xe[src]
            vals, mx, am, fl = h.acq(acq, par, float(y.min()), Xe)
            want = _lib.acq_from_moments(ctx, acq, par, float(y.min()), *h.predict(Xe))
            assert _bits(vals, want[0]) and _bits([mx], [want[1]]) and (am, fl) == want[2:], (kind, acq, edit)
            assert h.acq(acq, par, float(y.min()), Xe, want_values=False)[1:] == (mx, am, fl) or np.isnan(mx)
            assert np.isnan(vals[am]) if np.isnan(vals).any() else am == int(np.argmax(vals))
    h.close()


@pytest.mark.parametrize("kind,D,F", [("given", 1, 17), ("linear", 3, 4), ("quadratic", 3, 7), ("rff", 3, 128)])
def test_fused(ctx, kind, D, F):
    _check_fused(ctx, kind, D, F, 401)


def test_refusals(ctx):
    om, ph = np.ones((65, 129)), np.ones(129)
    for kind, D, F in (("given", 1, 0), ("given", 1, 129), ("linear", 65, 66), ("rff", 65, 8), ("rff", 2, 129), ("linear", 3, 5)):
        with pytest.raises(ValueError):
            _lib.DeviceBLR(ctx, kind, D, F, omega=om[:D, :F], phase=ph[:F], scale=1.0)
    h = _lib.DeviceBLR(ctx, "linear", 2, 3)
    for call in (lambda: h.predict(np.zeros((4, 2))), lambda: h.set_hypers(np.ones((1, 2))), lambda: h.loglik(np.zeros((1, 2)))):
        with pytest.raises(Exception, match="trained first"):
            call()
    h.set_data(np.random.RandomState(0).rand(9, 2), np.arange(9.0))
    for ab in (np.ones((0, 2)), np.ones((65, 2)), np.array([[1.0, -1.0]]), np.array([[np.nan, 1.0]])):
        with pytest.raises(ValueError):
            h.set_hypers(ab)
    with pytest.raises(ValueError):
        h.loglik(np.zeros((1, 2)), form=2)
    h.close()


@pytest.mark.parametrize("name,basis", [("linear", linear_basis_func), ("quadratic", quadratic_basis_func),
                                        ("quadratic", lambda x: quadratic_basis_func(x))])
def test_class_golden(ctx, name, basis, monkeypatch):
    """the reference's class on its own numbers (tests/golden/ref_blr.npz), the likelihood's form 0 included; EI, LogEI, PI
    and LCB over the model answer from the fused call alone (predict is taken away)"""
    gold, (X, y, Xt) = np.load(GOLDEN), inputs()
    model = BayesianLinearRegression(alpha=1, beta=1000, basis_func=basis, rng=np.random.RandomState(1), ctx=ctx)
    model.train(X, y, do_optimize=False)
    F = basis(X).shape[1]
    mean, var = model.predict(Xt)
    assert np.allclose(mean, gold[name + "_mean"], rtol=1e-9, atol=1e-11) and np.allclose(var, gold[name + "_var"], rtol=1e-9)
    m, S = model.models[0]
    assert np.allclose(basis(Xt).dot(m), mean, rtol=1e-9, atol=1e-11) and S.shape == (F, F) and model.hypers == [[1, 1000]]
    model.prior = None
    for t, ref in zip(THETAS, gold[name + "_mll"]):
        assert abs(model.marginal_log_likelihood(t) - ref) <= C_LL * F * EPS * (abs(ref) + np.exp(t[1]) * float(y @ y))
    monkeypatch.setattr(model, "predict", None)
    for cls, kind, par in ((EI, "ei", 0.0), (LogEI, "log_ei", 0.01), (PI, "pi", 0.0), (LCB, "lcb", 2.0)):
        want = _lib.acq_from_moments(ctx, kind, par, float(y.min()), mean, var)
        acq = cls(model, par=par)
        assert acq.argmax(Xt) == want[2] and acq.last_max == want[1] and _bits(np.ravel(acq.compute(Xt)), want[0])


def test_mcmc_replay(ctx):
    """do_mcmc=True: every likelihood the sampler was fed is the device's for that proposal (plus the host's prior), and the
    chain is the one a plain NumPy stretch move makes from those doubles, accept decision by accept decision"""
    X, y, _ = inputs()
    k, steps = 6, (3, 5)
    model = BayesianLinearRegression(basis_func=RandomFourierBasis("rbf", 2, 40, 0.5, np.random.RandomState(2)), n_hypers=k,
                                     burnin_steps=steps[0], chain_length=steps[1], rng=np.random.RandomState(3),
                                     exact_mll=True, ctx=ctx)
    fed, inner, rs = [], model._lnprob_batch, np.random.RandomState(3)     # (the sampler's stream starts as the model's)
    model._lnprob_batch = lambda th: fed.append((th.copy(), inner(th))) or fed[-1][1].copy()   # (the sampler writes into it)
    model.train(X, y)
    for th, ll in fed:
        assert ll.shape == (len(th),) and _bits(ll, model._dev.loglik(th, 1) + np.array([model.prior.lnprob(t) for t in th]))
    calls, p, halves = iter(fed), fed[0][0].copy(), (slice(k // 2), slice(k // 2, k))
    for n_steps in steps:
        th, lnp = next(calls)
        assert _bits(th, p)
        lnp = lnp.copy()
        for _ in range(n_steps):
            for own, other in (halves, halves[::-1]):
                z = (rs.rand(k // 2) + 1.0) ** 2 / 2.0
                partner = p[other][rs.randint(k // 2, size=k // 2)]
                q = partner - z[:, None] * (partner - p[own])
                th, new = next(calls)
                assert _bits(th, q)
                accept = np.log(z) + new - lnp[own] > np.log(rs.rand(k // 2))
                p[own], lnp[own] = np.where(accept[:, None], q, p[own]), np.where(accept, new, lnp[own])
    assert next(calls, None) is None and model.burned and _bits(model.p0, p) and _bits(model.hypers, np.exp(p))
    assert len(model.models) == k and np.all(model.predict(X)[1] >= EPS)


def test_rff_against_exact_gp(ctx):
    """A sanity check, N = 3000, D = 3, F = 128: BLR on random Fourier features of the RBF kernel against the exact GP with
    that kernel (oracle.gp_oracle; amplitude 1 / alpha, noise 1 / beta) on a smooth function.  The gap is the feature
    approximation's, not rounding, so no tolerance of tests/_tol.py applies: it is measured and written down (largest
    |mean_blr - mean_gp| over 200 points: interpreter 0.0465, MI355X 0.0465; NOTES.md).  Asserted is only that the gap stays
    below the noise's standard deviation, 0.1: an approximation further from the exact model than the data's own scatter is none."""
    rs = np.random.RandomState(5)
    N, D, F, ls, alpha, beta = 3000, 3, 128, 0.7, 1.0, 100.0
    X, Xt = rs.rand(N, D), rs.rand(200, D)
    y = np.sin(3 * X[:, 0]) * np.cos(2 * X[:, 1]) + X[:, 2] ** 2 + 0.1 * rs.randn(N)
    model = BayesianLinearRegression(alpha=alpha, beta=beta, basis_func=RandomFourierBasis("rbf", D, F, ls, rs), ctx=ctx)
    model.train(X, y, do_optimize=False)
    theta = np.array([-np.log(alpha)] + [2 * np.log(ls)] * D + [-np.log(beta)])
    mu = gp_oracle.gp_predict_diag("rbf", theta, gp_oracle.gp_compute("rbf", theta, X), X, y, 0.0, Xt)[0]
    gap = float(np.max(np.abs(model.predict(Xt)[0] - mu)))
    print("blr rff: largest |mean_blr - mean_gp| %.3g" % gap)
    assert gap < 0.1


def test_front_end(emu_ctx):
    """bayesian_optimization(model_type="blr"): five iterations on Branin, one objective call each; the reference's module
    path resolves to this package's through compat.install()"""
    from robo_amd import compat
    from robo_amd.fmin import bayesian_optimization
    calls = []

    def branin(x):
        calls.append(x.copy())
        a, b = x[0], x[1]
        return (b - 5.1 / (4 * np.pi ** 2) * a ** 2 + 5 / np.pi * a - 6) ** 2 + 10 * (1 - 1 / (8 * np.pi)) * np.cos(a) + 10

    res = bayesian_optimization(branin, np.array([-5.0, 0.0]), np.array([10.0, 15.0]), num_iterations=5, model_type="blr",
                                acquisition_func="ei", n_candidates=200, chain_length=4, burnin_steps=4,
                                rng=np.random.RandomState(4))
    assert len(calls) == 5 and len(res["y"]) == 5 and res["f_opt"] == min(res["y"])
    for model_type in ("dngo", "rf", "bohamiann"):
        with pytest.raises(ValueError):
            bayesian_optimization(branin, np.array([-5.0, 0.0]), np.array([10.0, 15.0]), num_iterations=5, model_type=model_type)
    compat.install(force=True)
    try:
        import robo.models.bayesian_linear_regression as ref_path
        assert ref_path.BayesianLinearRegression is BayesianLinearRegression
    finally:
        compat.uninstall()


@pytest.mark.gpu
def test_large_gpu(gpu_ctx):
    """N = 2^18, F = 128 random Fourier features in D = 3 -- the shape the exact fit cannot take -- and 32 773 / 65 536 fused"""
    _check_fused(gpu_ctx, "rff", 3, 128, 32768 + 5)
    N, D, F, m = 1 << 18, 3, 128, 1 << 16
    h, X, y, _, feat = _model(gpu_ctx, "rff", D, F, N)
    Phi = feat["scale"] * np.cos(X @ feat["omega"] + feat["phase"])
    A = np.abs(Phi)
    dphi = feat["scale"] * EPS * (2 + (D + 2) * (np.abs(X) @ np.abs(feat["omega"]) + np.abs(feat["phase"])))
    bound = (C + N // C) * EPS * (A.T @ A) + dphi.T @ A + A.T @ dphi
    assert np.all(np.abs(h.stats()[0] - Phi.T @ Phi) <= bound)
    h.set_hypers(np.exp(np.random.RandomState(1).uniform(-2, 6, (20, 2))))
    Xc = np.random.RandomState(2).rand(m, D) * 2.0 - 0.6
    vals, mx, am, fl = h.acq("ei", 0.0, float(y.min()), Xc)
    want = _lib.acq_from_moments(gpu_ctx, "ei", 0.0, float(y.min()), *h.predict(Xc))
    assert _bits(vals, want[0]) and am == int(np.argmax(vals)) == want[2] and mx == vals[am] and fl == want[3]
    h.close()
