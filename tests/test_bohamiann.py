"""BOHAMIANN: the SGHMC chains and the ensemble sweep (robo_amd/csrc/bnn.hip, api_bnn.hip) and models/bohamiann.py against the
plain long-double oracle of tests/bohamiann_oracle.py.  CPU: through the interpreter (tests/hipemu).  -m gpu: the same checks
on the MI355X, plus one default-length run and a fused sweep over 65 536 candidates.

Bounds, derived (eps = 2^-52, |.| entrywise; dg, dV .. are bounds on the device's error in g, V ..):
  gradient   dg = c eps S, c = batch + L (max(dim, H) + 2) + 8: test_dngo.py's bound with the batch as the only row sum and no
             chunks, plus exp(-l), its product with the error and the division by |B| (4 roundings, doubled); S the oracle's
             sum of the absolute values of the terms.  g itself is not an output: it is checked through gbar, V and v.
  burn-in    from the device's own state before the step: tau has no g in it, 5 roundings: 8 eps (|tau| + 1 + |tau gbar^2 / V|);
             gbar: r dg + 6 eps (|gbar| + r (|g| + |gbar|));  V: r (2 |g| dg + dg^2) + 6 eps (|V| + r (g^2 + |V|)).  After the
             burn-in tau, gbar and V must not move: bit for bit.
  velocity   with M and sigma in long double from the device's NEW V: eps2 M dg + |xi| dsigma + 8 eps (|v| + eps2 M |g| +
             mdecay |v| + sigma |xi|), dsigma = 4 eps (c2 M + eps4) / (2 sigma) + 2 eps sigma (sigma >= 1e-8: the clamp).
  parameter  p' = fl(p + v') of the device's own v': half an ulp, eps |p'|.
  normals    log, sqrt and cos are within 2 ulp each on either side, 2 pi u2 carries one rounding of an angle below 2 pi whose
             cosine moves by at most that: |xi - xi_orc| <= 16 eps rad, rad = sqrt(-2 log(1 - u1)); through one step this is
             sigma times that plus an ulp of v'.  The indices are exact, or g and with it v' move by far more.
  sweep      every sample's value within test_dngo.py's forward bound df; with D = max_s df, fmax = max_s |f_s| and
             E = D + (S + 4) eps fmax (Welford's running mean carries S roundings of values below fmax): |mean| within E,
             the variance within 4 a E + 4 E^2 + (S + 8) eps var, a = mean_s |f_s - mean|.
Largest error / bound observed (NOTES.md): step 0.50 on the interpreter and on the MI355X (the parameter's half ulp against a
bound of one), device draws 0.49 / 0.49, the sweep's mean 0.048 / 0.037.
"""
import os
import sys

import numpy as np
import pytest

from robo_amd import _lib
from robo_amd.acquisition_functions import EI, LCB, PI, LogEI
from robo_amd.models import Bohamiann, WrapperBohamiann
from robo_amd.models.bohamiann import kaiming_params

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bohamiann_oracle as BO  # noqa: E402
import dngo_oracle as O  # noqa: E402
from test_dngo import _forward_bound  # noqa: E402
from test_ehvi import _bits, emu_ctx, gpu_ctx  # noqa: E402,F401

LD, EPS = BO.LD, BO.EPS
PRIOR = (1e-6, 0.01, 1.0)
SHAPES = [(1, 1, 1, 1, 1, 1), (33, 3, 15, 2, 16, 1), (33, 17, 16, 3, 17, 3), (40, 64, 17, 1, 20, 1), (40, 3, 50, 2, 20, 2),
          (70, 17, 64, 3, 64, 1)]


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def ctx(request):
    return request.getfixturevalue(request.param + "_ctx")


def _problem(ctx, n, dim, H, L, batch, C, T=0):
    """chains with start parameters, data and the caller's draws for T steps"""
    rs = np.random.RandomState(n + dim + H)
    X = rs.rand(n, dim) * 2.0 - 0.6
    y = np.sin(3 * X[:, 0]) + X[:, -1] ** 2 + 0.1 * rs.randn(n)
    bnn = _lib.DeviceBNN(ctx, dim, L, H, C)
    start = np.stack([kaiming_params(rs, dim, L, H) for _ in range(C)])
    start[:, :-1] += 0.05 * rs.randn(C, bnn.n_params - 1)         # biases off zero
    bnn.set_state(start)
    return bnn, X, y, start, rs.randint(0, n, (T, batch)).astype(np.int32), rs.randn(T, C, bnn.n_params)


def _check_steps(trace, idx, xi, X, y, shape, burn, lr, mdecay, t0=0, dxi=None):
    """every step of the trace against the oracle from the device's own state -> largest error / bound"""
    n, dim, H, L, batch, C = shape
    cg, worst, clamped = (batch + L * (max(dim, H) + 2) + 8) * EPS, 0.0, False
    for t in range(len(idx)):
        for c in range(C):
            row, nxt = np.asarray(trace[t, c], dtype=LD), np.asarray(trace[t + 1, c], dtype=LD)
            rows = idx[t] if idx.ndim == 2 else idx[t, c]
            g, ga = BO.grad(row[0], dim, L, H, X[rows], y[rows], n, *PRIOR)
            dg, (p, v, tau, gbar, V) = cg * ga, row
            if t0 + t < burn:
                r = 1 / (tau + 1)
                want = BO.step(row, g, xi[t, c], True, lr, n, mdecay)
                bounds = (8 * EPS * (np.abs(tau) + 1 + np.abs(tau * gbar * gbar / V)),
                          r * dg + 6 * EPS * (np.abs(gbar) + r * (np.abs(g) + np.abs(gbar))),
                          r * (2 * np.abs(g) * dg + dg * dg) + 6 * EPS * (np.abs(V) + r * (g * g + np.abs(V))))
                for a, b in zip((2, 3, 4), bounds):
                    worst = max(worst, float(np.max(np.abs(nxt[a] - want[a]) / b)))
            else:
                assert _bits(trace[t + 1, c, 2:], trace[t, c, 2:]), (t, c)
            vo, e2m, sig, raw, unit = BO.velocity(v, g, xi[t, c], nxt[4], lr, n, mdecay)
            clamped = clamped or bool(np.any(raw < 1e-16))
            dsig = 4 * EPS * unit / (2 * sig) + 2 * EPS * sig
            dv = e2m * dg + np.abs(xi[t, c]) * dsig + 8 * EPS * (np.abs(v) + e2m * np.abs(g) + mdecay * np.abs(v) + sig * np.abs(xi[t, c]))
            dv = dv if dxi is None else dv + sig * dxi[t, c]
            worst = max(worst, float(np.max(np.abs(nxt[1] - vo) / dv)))
            worst = max(worst, float(np.max(np.abs(nxt[0] - (p + nxt[1])) / (EPS * np.abs(nxt[0]) + 1e-300))))
    return worst, clamped


@pytest.mark.parametrize("dim,H,L", [(3, 5, 2), (2, 4, 3)])
def test_oracle_gradient(dim, H, L):
    """the oracle's dU / d(p, l) against central differences of the oracle's potential in long double, h = 2^-21: the rounding
    error of the quotient is 2^-63 |U| / h per evaluation (times 8 for the sums inside U), the truncation error h^2 |U'''| / 6
    taken as h^2 max |g|"""
    rs = np.random.RandomState(dim)
    X, y = rs.rand(9, dim) * 2.0 - 0.6, rs.randn(9)
    pl = np.asarray(kaiming_params(rs, dim, L, H) + 0.3 * rs.randn((dim + 1) * H + (L - 1) * (H + 1) * H + H + 2), dtype=LD)
    h = LD(2) ** -21
    fd = [(BO.potential(pl + h * u, dim, L, H, X, y, 40, *PRIOR) - BO.potential(pl - h * u, dim, L, H, X, y, 40, *PRIOR)) / (2 * h)
          for u in np.eye(pl.size, dtype=LD)]
    g = BO.grad(pl, dim, L, H, X, y, 40, *PRIOR)[0]
    # exp(-l) = 100 scales U and g: the bound is test_dngo.py's, written in |U| and max |g| instead of for |loss| about 1
    bound = 8 * LD(2) ** -63 * abs(BO.potential(pl, dim, L, H, X, y, 40, *PRIOR)) / h + h * h * np.max(np.abs(g))
    assert np.max(np.abs(g)) > 1e-2 and bound < 1e-8 and np.all(np.abs(g - np.array(fd)) <= bound)


@pytest.mark.parametrize("shape,burn,lr,mdecay,edge", [(s, 3, 1e-2, 0.05, "") for s in SHAPES] + [
    (SHAPES[1], 0, 1e-2, 0.05, "no burn-in"), (SHAPES[2], 3, 1e-2, 0.05, "repeat"), (SHAPES[1], 3, 0.5, 1e-3, "clamp")])
def test_every_step(ctx, shape, burn, lr, mdecay, edge):
    T = 6
    bnn, X, y, start, idx, xi = _problem(ctx, *shape, T=T)
    if edge == "repeat":
        idx[:, 1] = idx[:, 0]
    trace = bnn.run(X, y, T, burn, 2, shape[4], lr, mdecay, *PRIOR, idx=idx, xi=xi, want_trace=True)
    assert _bits(trace[0, :, 0], start) and _bits(trace[0, :, 1], np.zeros_like(start)) and _bits(trace[0, :, 2:], np.ones((shape[5], 3, start.shape[1])))
    worst, clamped = _check_steps(trace, idx, xi, X, y, shape, burn, lr, mdecay)
    print("step error / bound %.3g" % worst)
    assert worst <= 1.0 and clamped == (edge == "clamp")
    bnn.close()


def test_invariances(ctx):
    """bit for bit: a then b is a + b; a run split across the launch bound; chain c of C alone; the kept samples"""
    shape, T, burn, keep = SHAPES[2], 7, 3, 2
    bnn, X, y, start, idx, xi = _problem(ctx, *shape, T=T)
    args = (burn, keep, shape[4], 1e-2, 0.05) + PRIOR
    ref = bnn.run(X, y, T, *args, idx=idx, xi=xi, want_trace=True)
    kept = np.concatenate((ref[5, :, 0], ref[7, :, 0]))            # step counts 5 and 7, chain-major inside a step
    assert _bits(bnn.samples, kept)
    bnn.set_state(start)
    first = bnn.run(X, y, 3, *args, idx=idx[:3], xi=xi[:3], want_trace=True)
    second = bnn.run(X, y, 4, *args, idx=idx[3:], xi=xi[3:], want_trace=True)
    assert _bits(np.concatenate((first, second[1:])), ref) and _bits(bnn.samples, kept)
    bnn.set_state(start)
    ctx.set_tuning("bnn_launch_steps", 2)
    try:
        assert _bits(bnn.run(X, y, T, *args, idx=idx, xi=xi, want_trace=True), ref) and _bits(bnn.samples, kept)
    finally:
        ctx.set_tuning("bnn_launch_steps", None)
    bnn.close()
    alone = _lib.DeviceBNN(ctx, shape[1], shape[3], shape[2], 1)
    alone.set_state(start[1:2])
    assert _bits(alone.run(X, y, T, *args, idx=idx, xi=xi[:, 1:2], want_trace=True)[:, 0], ref[:, 1])
    alone.close()


def test_table_cap(ctx):
    n, dim, H, L, batch, C = 33, 3, 15, 2, 16, _lib.BNN_MAX_CHAINS
    bnn, X, y, _, idx, xi = _problem(ctx, n, dim, H, L, batch, C, T=9)
    trace = bnn.run(X, y, 9, 0, 1, batch, 1e-2, 0.05, *PRIOR, idx=idx, xi=xi, want_trace=True)
    assert _bits(bnn.samples, trace[1:, :, 0].reshape(9 * C, -1)[:_lib.BNN_MAX_SAMPLES])     # 576 kept, 512 held
    bnn.close()


def test_device_draws(ctx):
    """idx and xi NULL: a traced run behind two untraced steps against the oracle's Philox draws of the same counters, then
    chain 0's first step replayed through the caller's-draws path"""
    shape, a, T, seed = (33, 17, 16, 3, 17, 2), 2, 3, 0x1234567887654321
    n, dim, H, L, batch, C = shape
    args = (1, 1, batch, 1e-2, 0.05) + PRIOR
    bnn, X, y, start, _, _ = _problem(ctx, *shape)
    bnn.run(X, y, a, *args, seed=seed)
    trace = bnn.run(X, y, T, *args, seed=seed, want_trace=True)
    idx = np.array([[BO.draw_indices(seed, a + t, c, batch, n) for c in range(C)] for t in range(T)])
    draws = [[BO.draw_normals(seed, a + t, c, bnn.n_params) for c in range(C)] for t in range(T)]
    xi, rad = (np.array([[d[k] for d in row] for row in draws], dtype=LD) for k in (0, 1))
    worst, _ = _check_steps(trace, idx, xi, X, y, shape, 1, 1e-2, 0.05, t0=a, dxi=16 * EPS * rad)
    print("device draws: step error / bound %.3g" % worst)
    assert worst <= 1.0
    bnn.close()
    one = _lib.DeviceBNN(ctx, dim, L, H, 1)
    one.set_state(start[:1])
    own = one.run(X, y, 1, *args, seed=seed, want_trace=True)
    one.set_state(start[:1])
    xi0, rad0 = BO.draw_normals(seed, 0, 0, one.n_params)
    fed = one.run(X, y, 1, *args, idx=BO.draw_indices(seed, 0, 0, batch, n)[None], xi=np.asarray(xi0, dtype=np.float64)[None, None],
                  want_trace=True)
    sig = BO.velocity(fed[0, 0, 1], 0, xi0, fed[1, 0, 4], 1e-2, n, 0.05)[2]
    assert _bits(own[1, 0, 2:], fed[1, 0, 2:])                    # the same rows: the same g, bit for bit
    assert np.all(np.abs(own[1, 0, 1] - fed[1, 0, 1]) <= sig * 17 * EPS * rad0 + 2 * EPS * np.abs(fed[1, 0, 1]))
    one.close()


def _samples(rs, dim, L, H, S):
    return np.stack([kaiming_params(rs, dim, L, H, log_noise=rs.randn() - 3.0) for _ in range(S)]) + \
        np.append(0.1 * rs.randn((dim + 1) * H + (L - 1) * (H + 1) * H + H + 1), 0.0)


@pytest.mark.parametrize("dim,H,L,S", [(1, 1, 1, 1), (3, 15, 2, 2), (17, 16, 3, 1), (64, 17, 1, 2), (3, 50, 2, 100), (17, 64, 3, 2)])
def test_sweep(ctx, dim, H, L, S):
    rs = np.random.RandomState(dim + H + S)
    samples, X = _samples(rs, dim, L, H, S), rs.rand(401, dim) * 2.0 - 0.6
    bnn = _lib.DeviceBNN(ctx, dim, L, H)
    bnn.set_samples(samples)
    mean, var, ps = bnn.predict(X, per_sample=True)
    mo, vo, fo = BO.predict(samples, dim, L, H, X)
    D = np.max([_forward_bound(s[:-1], dim, L, H, X)[1] for s in samples], axis=0)
    E = D + (S + 4) * EPS * np.abs(fo).max(axis=0)
    dvar = 4 * np.abs(fo - mo).mean(axis=0) * E + 4 * E * E + (S + 8) * EPS * vo
    print("sweep error / bound: mean %.3g" % float(np.max(np.abs(mean - mo) / E)))
    assert np.all(np.abs(mean - mo) <= E)
    if S == 1:
        assert _bits(var, np.full(401, EPS))                     # exactly 0 before the clip
    else:
        assert np.all(np.abs(var - vo) <= dvar) and np.all(var > EPS)
    mlp = _lib.DeviceMLP(ctx, dim, L, H)                          # every sample's values: robo_mlp_forward's bits
    for s in (0, S - 1):
        mlp.set_params(samples[s, :-1])
        assert _bits(ps[s], mlp.forward(X)[1])
    mlp.close()
    for m in (1, 63, 64, 65):                                     # other batch sizes and positions: the same bits
        assert all(_bits(u, w[:m]) for u, w in zip(bnn.predict(X[:m]), (mean, var))), m
    back = bnn.predict(np.concatenate((X[:3], X[::-1])))
    assert _bits(back[0][3:][::-1], mean) and _bits(back[1][3:][::-1], var)
    bad = bnn.predict(np.where(np.arange(dim) == dim - 1, np.nan, X[:2]))
    assert np.all(np.isnan(bad[0])) and np.all(np.isnan(bad[1]))
    for acq, par in (("ei", 0.0), ("log_ei", 0.01), ("pi", 0.0), ("lcb", 2.0)):
        vals, mx, am, fl = bnn.acq(acq, par, float(mean.min()), X)
        want = _lib.acq_from_moments(ctx, acq, par, float(mean.min()), mean, var)
        assert _bits(vals, want[0]) and _bits([mx], [want[1]]) and (am, fl) == want[2:], acq
    bnn.set_output_transform(1.5, 2.0, True)                      # the transform and the noise flag
    tm, tv = bnn.predict(X)
    noise = np.exp(np.asarray(samples[:, -1], dtype=LD)).mean()
    raw = np.where(S == 1, 0.0, var)
    assert _bits(tm, mean * 2.0 + 1.5) and np.all(np.abs(tv - 4 * (raw + noise)) <= 4 * (dvar + (S + 8) * EPS * (vo + noise)))
    bnn.close()


def test_refusals(ctx):
    for dim, L, H, C in ((0, 1, 4, 1), (65, 1, 4, 1), (2, 0, 4, 1), (2, 4, 4, 1), (2, 1, 0, 1), (2, 1, 65, 1), (2, 1, 4, 0), (2, 1, 4, 65)):
        with pytest.raises(ValueError):
            _lib.DeviceBNN(ctx, dim, L, H, C)
    bnn, X, y = _lib.DeviceBNN(ctx, 2, 2, 5, 2), np.random.RandomState(0).rand(9, 2), np.arange(9.0)
    for call in (lambda: bnn.run(X, y, 1, 0), lambda: bnn.predict(X), lambda: bnn.acq("ei", 0.0, 0.0, X)):
        with pytest.raises(Exception, match="trained first"):
            call()
    start = np.stack([kaiming_params(np.random.RandomState(c), 2, 2, 5) for c in range(2)])
    with pytest.raises(ValueError):
        bnn.set_state(np.where(np.arange(start.shape[1]) == 3, np.nan, start))
    bnn.set_state(start)
    ok = dict(n_steps=1, n_burn_in=0, keep_every=1, batch=4, lr=0.01, mdecay=0.05, prior_mu=1e-6, prior_s=0.01, prior_lambda=1.0)
    for bad in (dict(n_steps=-1), dict(n_burn_in=-1), dict(keep_every=0), dict(batch=0), dict(batch=65), dict(lr=0.0),
                dict(lr=np.inf), dict(lr=np.nan), dict(mdecay=0.0), dict(mdecay=np.nan), dict(prior_mu=0.0), dict(prior_s=-1.0),
                dict(prior_lambda=-1.0), dict(prior_lambda=np.inf), dict(idx=np.full((1, 4), 9)), dict(idx=np.full((1, 4), -1))):
        with pytest.raises(ValueError):
            bnn.run(X, y, **dict(ok, **bad))
    for call in (lambda: bnn.run(X[:0], y[:0], 1, 0), lambda: bnn.run(X, np.where(np.arange(9) == 4, np.nan, y), 1, 0),
                 lambda: bnn.set_samples(np.full((1, bnn.n_params), np.inf)), lambda: bnn.set_samples(np.zeros((513, bnn.n_params))),
                 lambda: bnn.set_output_transform(0.0, 0.0), lambda: bnn.set_output_transform(np.nan, 1.0)):
        with pytest.raises(ValueError):
            call()
    so = _lib.lib()                                              # every NULL required pointer
    for status in (so.robo_bnn_run(bnn._h, None, None, 9, 1, 0, 1, 4, 0.01, 0.05, 1e-6, 0.01, 1.0, 0, None, None, None, None),
                   so.robo_bnn_set_state(bnn._h, None), so.robo_bnn_set_samples(bnn._h, 1, None),
                   so.robo_bnn_param_count(bnn._h, None), so.robo_bnn_get_samples(bnn._h, None, None),
                   so.robo_bnn_predict(bnn._h, None, 9, None, None, None), so.robo_bnn_create(ctx._h, 2, 1, 4, 1, None)):
        assert status == _lib.BAD_ARGUMENT
    bnn.run(X, y, 2, 0, 1, 4)                                     # two good steps: four samples
    kept = bnn.samples
    with pytest.raises(FloatingPointError) as err:               # a run that diverges: its earlier samples stay
        bnn.run(X, 1e200 * (y + 1), 8, 0, 1, 4, lr=1e150)
    assert err.value.status.max() == 1 and _bits(bnn.samples[:4], kept) and len(kept) == 4
    with pytest.raises(Exception, match="trained first"):         # the chains ended: a new start state comes first
        bnn.run(X, y, 1, 0)
    bnn.close()


def test_class(ctx, monkeypatch):
    """Bohamiann on a 1-D toy: the kept samples are the oracle's replay of the same draws; predict is the oracle's mixture
    of the device's samples; EI, LogEI, PI and LCB answer from the fused call alone (predict is taken away)"""
    rs = np.random.RandomState(3)
    X = rs.rand(30, 1) * 3.0
    y = 2.0 * np.sin(3 * X[:, 0]) + 5.0 + 0.05 * rs.randn(30)
    with pytest.raises(ValueError):
        WrapperBohamiann(get_net=lambda d: None)
    model = WrapperBohamiann(get_net=(2, 16), n_burn_in=60, n_steps=120, keep_every=20, rng=np.random.RandomState(1), ctx=ctx)
    assert isinstance(model, Bohamiann) and Bohamiann().n_units == (50, 50) and Bohamiann().n_chains == 1
    model.train(X, y)
    Xn, yn = (X - X.mean(axis=0)) / X.std(axis=0), (y - y.mean()) / y.std()
    row, kept = np.stack([model.start[0]] + [0 * model.start[0]] + 3 * [1 + 0 * model.start[0]]), []
    for t in range(120):
        idx = BO.draw_indices(model.seed, t, 0, 20, 30)
        g = BO.grad(row[0], 1, 2, 16, Xn[idx], yn[idx], 30, *PRIOR)[0]
        row = BO.step(row, g, BO.draw_normals(model.seed, t, 0, row.shape[1])[0], t < 60, 1e-2, 30, 0.05)
        if t + 1 > 60 and (t + 1 - 60) % 20 == 0:
            kept.append(row[0])
    # 120 steps, each contracting v by mdecay and moving p by eps^2 M g ~ 1e-4 g: rounding of 1e-16 per step cannot grow past 1e-12
    assert model.samples.shape == (3, row.shape[1]) and np.allclose(model.samples, np.asarray(kept, dtype=float), rtol=1e-9, atol=1e-11)
    Xt = np.linspace(0.0, 3.0, 65)[:, None]
    mean, var = model.predict(Xt)
    mo, vo, _ = BO.predict(model.samples, 1, 2, 16, (Xt - X.mean(axis=0)) / X.std(axis=0))
    assert mean.shape == var.shape == (65,) and np.allclose(mean, np.asarray(mo * y.std() + y.mean(), dtype=float), rtol=1e-12)
    assert np.allclose(var, np.asarray(vo * y.std() ** 2, dtype=float), rtol=1e-9, atol=1e-15) and model.get_incumbent()[1] == y.min()
    monkeypatch.setattr(model, "predict", None)
    for cls, kind, par in ((EI, "ei", 0.0), (LogEI, "log_ei", 0.01), (PI, "pi", 0.0), (LCB, "lcb", 2.0)):
        want = _lib.acq_from_moments(ctx, kind, par, float(y.min()), mean, var)
        acq = cls(model, par=par)
        assert _bits(np.ravel(acq.compute(Xt)), want[0]) and acq.argmax(Xt) == want[2] and acq.last_max == want[1]


def test_solver(ctx):
    """three iterations of the solver on Branin with Bohamiann and EI call the objective once each"""
    from robo_amd.maximizers import RandomSampling
    from robo_amd.solver.bayesian_optimization import BayesianOptimization
    calls, lower, upper = [], np.array([-5.0, 0.0]), np.array([10.0, 15.0])

    def branin(x):
        calls.append(x)
        return (x[1] - 5.1 / (4 * np.pi ** 2) * x[0] ** 2 + 5 / np.pi * x[0] - 6) ** 2 + 10 * (1 - 1 / (8 * np.pi)) * np.cos(x[0]) + 10

    rng = np.random.RandomState(5)
    model = Bohamiann(n_units=(16, 16), n_burn_in=20, n_steps=60, keep_every=10, rng=rng, ctx=ctx)
    acq = EI(model)
    bo = BayesianOptimization(branin, lower, upper, acq, model, RandomSampling(acq, lower, upper, rng=rng, n_samples=200),
                              initial_points=3, rng=rng)
    inc, val = bo.run(6)
    assert len(calls) == 6 and np.isfinite(val) and np.shape(inc) == (2,)


@pytest.mark.gpu
def test_default_run_gpu(gpu_ctx):
    """n = 200, D = 16, the default net and schedule (30 000 steps), then a fused sweep of 65 536 candidates: it completes, is
    finite and reproduces under the same seed"""
    rs = np.random.RandomState(0)
    X = rs.rand(200, 16)
    y = np.sin(3 * X[:, 0]) + X[:, 1] ** 2 + 0.1 * rs.randn(200)
    Xc, out = rs.rand(1 << 16, 16), []
    for _ in range(2):
        model = Bohamiann(rng=np.random.RandomState(7), ctx=gpu_ctx)
        model.train(X, y)
        out.append((model.samples,) + model.acquisition("ei", 0.0, float(y.min()), Xc))
    assert out[0][0].shape[0] == 100 and np.all(np.isfinite(out[0][0])) and np.all(np.isfinite(out[0][1]))
    assert _bits(out[0][0], out[1][0]) and _bits(out[0][1], out[1][1]) and out[0][2:] == out[1][2:]


