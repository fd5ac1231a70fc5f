"""The device-resident CMA-ES maximiser (robo_amd/csrc/cmaes.hip, robo_acq_cmaes_cand / robo_acq_cmaes_marginal_cand,
ClosedFormAcquisition.cmaes, maximizers.CMAES) against tests/cmaes_oracle.py.

Trajectories are not compared.  Every generation of the device's trace is replayed on its own from the device's previous
state: x from the trace's z and the device's A, the repaired y from the device's x, the ranks bit for bit from the device's
values, then m, p_sigma, sigma, p_c and C from the device's y and ranks.  Bounds are forward-error bounds: a sum of k
terms evaluated in any order, fused or not, is off by at most k eps sum|terms|; every check allows (k + c) eps sum|terms|
with c <= 12 for the few roundings around the sum (scalings, the final add, sqrt and exp) plus the bound of the inputs it
is formed from, propagated through their coefficients (cmaes_oracle.py states each next to its formula).  A and A^-1 are
checked by what defines them; their residuals may be 8 times what NumPy's eigh-built root leaves on the same C (floor
D eps |C|_max).  Largest ratios observed: NOTES.md.  CPU: the interpreter; -m gpu: the MI355X, + one case at working size.
"""
import os
import sys

import numpy as np
import pytest

from robo_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cmaes_oracle as CO  # noqa: E402
from _tol import ACQ_RTOL, assert_logei_close  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402

ACQS = (("ei", 0.0), ("log_ei", 0.0), ("pi", 0.0), ("lcb", 1.0))
LOGEI = (("log_ei", 0.0),)
STEP_CASES = [(2, 4, 1, 1, LOGEI), (3, 6, 3, 1, ACQS), (16, 16, 2, 3, LOGEI), (17, 17, 2, 1, LOGEI), (5, 33, 1, 2, LOGEI)]


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


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def ctx(request):
    return request.getfixturevalue(request.param + "_ctx")


def _models(ctx, N, D, scales=(1.0,), seed=0):
    """the same GPs as oracles and on the device (inputs in [0, 1]^D) -> rs, oracle GPs, device GPs, y"""
    rs = np.random.RandomState(seed)
    X = rs.rand(N, D)
    y = np.sin(3 * X.sum(axis=1) / np.sqrt(D / 3.0)) + 0.1 * rs.randn(N)
    ogps, gps = [], []
    for f in scales:
        theta = np.concatenate([[0.0], np.log(np.full(D, 0.12 * D * f)), [np.log(1e-2)]])
        ogps.append(O.OracleGP("matern52", theta, normalize_input=False))
        ogps[-1].train(X, y)
        gps.append(_lib.DeviceGP(ctx, "matern52", N, D))
        gps[-1].set_data(X, y)
        gps[-1].fit(theta, ogps[-1].mean)
    return rs, ogps, gps, y


ORACLE_ACQ = {"ei": O.ei, "log_ei": O.log_ei_vec, "pi": O.pi}


def _values(ogps, kind, par, etas, P):
    mv = [g.predict(P, diag_only=True) for g in ogps]
    out = [O.lcb(m, v, par) if kind == "lcb" else ORACLE_ACQ[kind](m, v, eta, par) for (m, v), eta in zip(mv, etas)]
    return np.mean(np.array(out), axis=0), (etas[-1] - mv[-1][0] - par) / np.sqrt(mv[-1][1])


def _replay(tr, eig_every, ogps=None, kind=None, par=0.0, etas=None, gens=None):
    """every (generation, instance) of a trace against the oracle's step -> the largest error / bound ratio"""
    T1, R, L, D = tr["z"].shape
    K, worst, res = CO.constants(D, L), 0.0, 0.0
    for g in (range(T1 - 1) if gens is None else gens):
        for r in range(R):
            p, c = {k: v[g, r] for k, v in tr.items()}, {k: v[g + 1, r] for k, v in tr.items()}
            state = ("m", "sigma", "p_sigma", "p_c", "C", "A", "Ainv")
            if c["code"] in (6, 7):
                assert p["code"] != 0 and all(np.array_equal(p[k], c[k]) for k in state), (g, r)
                continue
            assert p["code"] == 0
            x, bound = CO.ask(p["m"], p["sigma"], p["A"], c["z"])
            finite = np.isfinite(c["z"]).all(axis=1)
            assert np.all(np.abs(c["x"] - x)[finite] <= bound[finite]) and np.all((c["x"] >= 0) & (c["x"] <= 1) | ~finite[:, None])
            y, bound = CO.repaired(c["x"], p["m"], p["sigma"])
            assert np.all(np.abs(c["y"] - y)[finite] <= bound[finite])
            np.testing.assert_array_equal(c["ranks"], CO.ranks(c["values"]))
            if c["code"] == 1:
                assert not np.isfinite(c["values"]).any() and all(np.array_equal(p[k], c[k]) for k in state), (g, r)
                continue
            out = CO.tell(K, g, p["m"], p["sigma"], p["p_sigma"], p["p_c"], p["C"], p["Ainv"], c["y"], c["ranks"], c)
            for k in ("m", "p_sigma", "sigma", "p_c", "C"):
                err, bound = np.abs(c[k] - out[k][0]).astype(np.float64), np.asarray(out[k][1], dtype=np.float64)
                assert np.all(err <= bound), (g, r, k, (err / bound).max())
                worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0)))
            assert out["h_sigma"][1] or c["h_sigma"] == out["h_sigma"][0], (g, r)
            assert np.array_equal(c["C"], c["C"].T)
            if c["code"] == 0 and (g + 1) % eig_every == 0:
                for M in (c["A"], c["Ainv"]):
                    assert np.array_equal(M, M.T)
                floor = D * CO.EPS * np.abs(c["C"]).max()
                got, ref = CO.sqrt_residuals(c["C"], c["A"], c["Ainv"]), CO.sqrt_residuals(c["C"], *CO.eigh_sqrt(c["C"]))
                for a, b, f in zip(got, ref, (floor, D * CO.EPS)):
                    assert a <= 8 * max(b, f), (g, r, a, b, f)
                    res = max(res, a / max(b, f))
                assert np.all(np.einsum("id,de,ie->i", c["y"], c["A"], c["y"])[np.abs(c["y"]).sum(axis=1) > 0] > 0)
            else:
                assert np.array_equal(c["A"], p["A"]) and np.array_equal(c["Ainv"], p["Ainv"])
            if ogps is not None:
                want, z = _values(ogps, kind, par, etas, c["x"])
                if kind == "log_ei" and len(ogps) == 1:
                    assert_logei_close(c["values"], want, z, rtol=ACQ_RTOL, tail_rtol=ACQ_RTOL)
                else:
                    np.testing.assert_allclose(c["values"], want, rtol=ACQ_RTOL, atol=0)
    print("largest error / bound %.3f, largest residual / yardstick %.3f" % (worst, res))
    return worst


def _steps(ctx, D, L, R, every, acqs, scales=(1.0,), N=60, T=8, M=40, z="draw", gens=None):
    rs, ogps, gps, y = _models(ctx, N, D, scales)
    etas = y.min() - 0.05 * np.arange(len(gps))
    cand = _lib.Candidates(ctx, rs.rand(M, D))
    zz = rs.randn(T, R, L, D) if z == "draw" else None
    try:
        for kind, par in acqs:
            vals, mx, am, _ = _lib.acq_marginal(gps, kind, par, etas, cand)
            r = _lib.cmaes_marginal(gps, kind, par, etas, cand, R, L, T, 0.3, eig_every=every, z=zz, seed=11, diagnostics=True)
            np.testing.assert_array_equal(r.trace["m"][0], cand.points()[np.argsort(-vals, kind="stable")[:R]])
            if zz is not None:
                np.testing.assert_array_equal(r.trace["z"][1:], zz)
            _replay(r.trace, every, ogps, kind, par, etas, gens)
            assert r.value >= mx and np.all((r.x >= 0) & (r.x <= 1))
            seen = r.trace["values"][1:][r.trace["code"][1:] < 6]          # (stopped instances' rows hold zeros)
            best = max(mx, seen[np.isfinite(seen)].max())
            assert r.value == best and r.value == _lib.cmaes_marginal(gps, kind, par, etas, cand, R, L, T, 0.3, eig_every=every,
                                                                      z=zz, seed=11).value
        return r, gps, cand, etas, zz
    finally:
        cand.close()
        for g in gps:
            g.close()


@pytest.mark.parametrize("D,L,R,every,acqs", STEP_CASES)
def test_every_step(ctx, D, L, R, every, acqs):
    _steps(ctx, D, L, R, every, acqs)


def test_marginal(ctx):
    _steps(ctx, 3, 6, 2, 1, (("log_ei", 0.0), ("ei", 0.01)), scales=(1.0, 0.6, 1.7))
    rs, ogps, gps, y = _models(ctx, 60, 3)
    cand, z = _lib.Candidates(ctx, rs.rand(40, 3)), rs.randn(4, 2, 6, 3)
    a = _lib.cmaes_marginal(gps, "log_ei", 0.0, y.min(), cand, 2, 6, 4, 0.3, z=z, diagnostics=True)
    b = gps[0].cmaes("log_ei", 0.0, y.min(), cand, 2, 6, 4, 0.3, z=z, diagnostics=True)
    assert all(a.trace[k].tobytes() == b.trace[k].tobytes() for k in a.trace) and (a.value, a.instance) == (b.value, b.instance)


def test_philox_draws(ctx):
    r = _steps(ctx, 5, 16, 3, 2, LOGEI, z=None, T=12)[0]
    zs = r.trace["z"][1:].ravel()
    n = zs.size
    assert abs(zs.mean()) <= 5 / np.sqrt(n) and abs(zs.var() - 1) <= 5 * np.sqrt(2.0 / n)
    assert len(np.unique(zs)) == n


def test_invariances(ctx):
    """one instance alone (its start as the only candidate, its own draws) is that instance among three, bit for bit; a
    handle that ran another (R, lambda) in between gives the bits of a fresh one; another seed gives other draws"""
    rs, ogps, (g, fresh), y = _models(ctx, 60, 3, (1.0, 1.0))
    Xc, z = rs.rand(40, 3), rs.randn(5, 3, 6, 3)
    cand = _lib.Candidates(ctx, Xc)

    def run(gp, c, R, zz, L=6, **how):
        return gp.cmaes("log_ei", 0.0, y.min(), c, R, L, 5, 0.3, z=zz, diagnostics=True, **how)
    three = run(g, cand, 3, z)
    for r in range(3):
        one = _lib.Candidates(ctx, three.trace["m"][0, r][None, :])
        alone = run(g, one, 1, z[:, r:r + 1])
        one.close()
        assert all(alone.trace[k][:, 0].tobytes() == three.trace[k][:, r].tobytes() for k in three.trace), r
    run(g, cand, 2, None, L=9)
    again, other = run(g, cand, 3, z), run(fresh, cand, 3, z)
    for a in (again, other):
        assert all(a.trace[k].tobytes() == three.trace[k].tobytes() for k in three.trace)
        assert (a.value, a.instance, a.flags, a.x.tobytes()) == (three.value, three.instance, three.flags, three.x.tobytes())
    s1, s1b, s2 = (run(g, cand, 2, None, seed=s).trace for s in (1, 1, 2))
    assert all(s1[k].tobytes() == s1b[k].tobytes() for k in s1) and not np.any(s1["z"][1:] == s2["z"][1:])


def test_edges(ctx, monkeypatch):
    D, L, T = 3, 6, 5
    rs, ogps, (g, fresh), y = _models(ctx, 60, D, (1.0, 1.0))
    eta, z = y.min(), rs.randn(T, 4, L, D)

    def run(c, R, zz, sigma0=0.3, **how):
        r = g.cmaes("log_ei", 0.0, eta, c, R, L, T, sigma0, z=zz, eig_every=1, diagnostics=True, **how)
        _replay(r.trace, 1)
        return r
    corner = _lib.Candidates(ctx, np.zeros((1, D)))
    r = run(corner, 1, z[:, :1], sigma0=2.0)               # nearly every sample is clipped; the replay checks x, y in the box
    x = r.trace["x"][1:]
    assert np.mean((x == 0) | (x == 1)) > 0.5 and np.all((r.trace["m"] >= 0) & (r.trace["m"] <= 1))
    corner.close()
    Xn = rs.rand(6, D)
    Xn[[0, 2, 3, 5], 0] = np.nan                           # NaN rows never start; two eligible rows for four instances
    few = _lib.Candidates(ctx, Xn)
    vals = g.acq("log_ei", 0.0, eta, few)[0]
    r = run(few, 4, z)
    order = [i for i in np.argsort(-vals, kind="stable") if not np.isnan(vals[i])]
    np.testing.assert_array_equal(r.trace["m"][0, :2], Xn[order])
    assert np.all(r.trace["code"][:, 2:] == 7) and np.all(r.trace["code"][:, :2] == 0) and r.instance in (0, 1)
    assert r.flags & _lib.FLAG_NAN and np.isfinite(r.value) and r.value >= np.nanmax(vals)
    few.close()
    cand = _lib.Candidates(ctx, rs.rand(40, D))
    zn = z[:, :2].copy()
    zn[2, 0] = np.nan                                      # every value of instance 0 is NaN in generation 2
    zn[:, 1, 1] = zn[:, 1, 0]                              # duplicated draws of instance 1: ties rank by index
    r = run(cand, 2, zn)
    np.testing.assert_array_equal(r.trace["code"][:, 0], [0, 0, 0, 1, 6, 6])
    assert r.flags & _lib.FLAG_FROZEN and r.flags & _lib.FLAG_NAN
    kept = max(g.acq("log_ei", 0.0, eta, cand, want_values=False)[1], r.trace["values"][1:3, 0].max())
    assert r.value == max(kept, r.trace["values"][1:, 1].max())
    assert np.all(r.trace["ranks"][1:, 1, 1] == r.trace["ranks"][1:, 1, 0] + 1)
    r = run(cand, 2, z[:, :2], sigma_min=10.0)             # sigma_min above sigma0: stops at generation 0
    np.testing.assert_array_equal(r.trace["code"][:, 0], [0, 5, 6, 6, 6, 6])
    assert r.flags & _lib.FLAG_FROZEN
    for kind, par in ACQS:                                 # T = 0: the sweep's argmax, point and value, bit for bit
        _, mx, am, fl = g.acq(kind, par, eta, cand, want_values=False)
        r0 = g.cmaes(kind, par, eta, cand, 3, L, 0, 0.3)
        assert (r0.value, r0.instance, r0.flags) == (mx, 0, fl) and np.array_equal(r0.x, cand.points()[am])
    other, one_d = _lib.Candidates(ctx, rs.rand(5, 2)), _lib.DeviceGP(ctx, "matern52", 5, 1)
    unfit, fab = _lib.DeviceGP(ctx, "matern52", 60, D), _lib.DeviceGP(ctx, "fabolas", 60, D)
    line = _lib.Candidates(ctx, rs.rand(5, 1))
    fab.set_data(rs.rand(60, D), y)
    fab.fit(np.concatenate([[0.0], np.log(np.full(D - 1, 0.4)), np.log([0.5, 0.8, 1e-2])]), 0.0)
    for bad in (dict(popsize=3), dict(popsize=65), dict(n_instances=0), dict(n_instances=65), dict(sigma0=0.0),
                dict(sigma0=np.inf), dict(sigma0=np.nan), dict(n_generations=-1), dict(gp=one_d, cand=line), dict(gp=fab),
                dict(eig_every=-1), dict(sigma_min=-1.0), dict(sigma_min=np.nan)):
        a = dict(dict(gp=g, cand=cand, n_instances=2, popsize=L, n_generations=2, sigma0=0.3), **bad)
        with pytest.raises(ValueError):
            a.pop("gp").cmaes("lcb", 1.0, 0.0, a.pop("cand"), **a)
    monkeypatch.setitem(_lib.ACQ_KINDS, "nothing", 9)                  # the library's own verdict on an unknown kind
    for call in (lambda: g.cmaes("nothing", 1.0, 0.0, cand), lambda: _lib.cmaes_marginal([g, g], "lcb", 1.0, 0.0, cand)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(_lib.RoboBadShape):
        g.cmaes("lcb", 1.0, 0.0, other, 2, L, 2)
    with pytest.raises(Exception, match="trained first"):
        unfit.cmaes("lcb", 1.0, 0.0, cand, 2, L, 2)
    ctx.set_tuning("ws_bytes", 1024)
    try:
        with pytest.raises(_lib.RoboBadShape):
            g.cmaes("lcb", 1.0, 0.0, cand, 2, L, 2)
    finally:
        ctx.set_tuning("ws_bytes", None)
    assert g.cmaes("lcb", 1.0, 0.0, cand, 2, L, 2).flags == 0          # the handle is still usable
    for h in (cand, other, line, one_d, unfit, fab, g, fresh):
        h.close()


def _bump_problem():
    """fixed 2-D data: a bowl around (0.86, 0.70) on a 6 x 6 grid gives LogEI a trend towards that corner of the box, a
    ring of 12 high observations of radius 0.2 around (0.84, 0.70) walls it off, and two low ones inside make the bump;
    64 candidates, none within 0.3 of it"""
    g1, a = np.linspace(0.0, 1.0, 6), 2 * np.pi * (np.arange(12) + 0.5) / 12
    X = np.array(np.meshgrid(g1, g1)).reshape(2, -1).T
    X = X + 0.02 * np.sin(7.0 * X[:, ::-1] + np.array([0.3, 1.1]))
    X = X[np.abs(X - np.array([0.84, 0.70])).max(axis=1) > 0.2]
    y = 3.0 + 8.0 * ((X - np.array([0.86, 0.70])) ** 2).sum(axis=1)
    X = np.vstack([X, np.array([0.84, 0.70]) + 0.2 * np.stack([np.cos(a), np.sin(a)], axis=1), [[0.80, 0.70], [0.84, 0.70]]])
    y = np.concatenate([y, np.full(12, 6.0), [0.0, -2.0]])
    c1 = (np.arange(8) + 0.5) / 8
    Xc = np.array(np.meshgrid(c1, c1)).reshape(2, -1).T
    Xc = Xc + 0.03 * np.cos(5.0 * Xc[:, ::-1] + np.array([0.7, 0.2]))
    near = np.abs(Xc - np.array([0.88, 0.70])).max(axis=1) < 0.3
    Xc[near] *= 0.3
    return X, y, np.concatenate([[0.0], np.log([0.01, 0.01]), [np.log(1e-4)]]), np.clip(Xc, 0.0, 1.0)


def test_finds_the_bump_the_candidates_miss(ctx):
    X, y, theta, Xc = _bump_problem()
    ogp = O.OracleGP("matern52", theta, normalize_input=False)
    ogp.train(X, y)
    t = np.linspace(0.0, 1.0, 257)
    fg = _values([ogp], "log_ei", 0.0, [y.min()], np.array(np.meshgrid(t, t)).reshape(2, -1).T)[0].reshape(257, 257)
    j, i = np.unravel_index(np.argmax(fg), fg.shape)
    xg, fc = np.array([t[i], t[j]]), _values([ogp], "log_ei", 0.0, [y.min()], Xc)[0]
    # the premise, from the oracle alone: a narrow bump (within 1 of the maximum on < 0.1 % of the grid, all of it next to
    # the maximum) far from every candidate and 30 above the best of them, whose hill is elsewhere
    top = np.argwhere(fg > fg.max() - 1.0)
    assert len(top) < 66 and np.all(np.abs(top - [j, i]) <= 8) and 0 < min(i, j) and max(i, j) < 256
    assert np.abs(Xc - xg).max(axis=1).min() > 0.25 and fg.max() - fc.max() > 30.0
    g = _lib.DeviceGP(ctx, "matern52", len(X), 2)
    g.set_data(X, y)
    g.fit(theta, ogp.mean)
    cand = _lib.Candidates(ctx, Xc)
    try:
        mx = g.acq("log_ei", 0.0, y.min(), cand, want_values=False)[1]
        ref = g.refine("log_ei", 0.0, y.min(), cand, 64, 60, 0.05)
        r = g.cmaes("log_ei", 0.0, y.min(), cand, 4, 12, 60, 0.25, z=np.random.RandomState(0).randn(60, 4, 12, 2))
        print("grid %.6f at %s, sweep %.6f, refine %.6f, cmaes %.6f at %s" % (fg.max(), xg, mx, ref.value, r.value, r.x))
        assert r.value > mx and r.value > ref.value
        assert np.abs(r.x - xg).max() <= t[1] and r.value >= fg[j - 1:j + 2, i - 1:i + 2].min()
    finally:
        cand.close()
        g.close()


def _branin(x):
    return float((x[1] - 5.1 / (4 * np.pi ** 2) * x[0] ** 2 + 5.0 / np.pi * x[0] - 6.0) ** 2 +
                 10.0 * (1 - 1.0 / (8 * np.pi)) * np.cos(x[0]) + 10.0)


def test_classes_and_front_end(ctx):
    import inspect
    from robo_amd.acquisition_functions import EI, InformationGain, LogEI, MarginalizationGPMCMC
    from robo_amd.fmin import bayesian_optimization
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.maximizers import CMAES
    from robo_amd.models import GaussianProcess
    lo, hi, rs = np.array([-5.0, 0.0]), np.array([10.0, 15.0]), np.random.RandomState(0)
    X = lo + (hi - lo) * rs.rand(12, 2)
    y = np.array([_branin(x) for x in X])

    def model(scale):
        m = GaussianProcess(2 * Matern52Kernel(np.full(2, scale), ndim=2), noise=1e-3, lower=lo, upper=hi,
                            rng=np.random.RandomState(3))
        m.train(X, y, do_optimize=False)
        return m

    class Mix(object):
        models = [model(0.3), model(0.2), model(0.5)]

        def get_incumbent(self):
            return self.models[0].get_incumbent()
    sig = inspect.signature(CMAES.__init__).parameters
    assert [(k, sig[k].default) for k in list(sig)[4:8]] == [("verbose", True), ("restarts", 0), ("n_func_evals", 1000),
                                                              ("rng", None)] and list(sig)[1:4] == ["objective_function", "lower", "upper"]
    for acq in (EI(model(0.3)), MarginalizationGPMCMC(LogEI(Mix()))):
        mx = CMAES(acq, lo, hi, verbose=False, restarts=2, n_func_evals=60, n_samples=200, rng=np.random.RandomState(5))
        x = mx.maximize()
        assert x.shape == (2,) and np.all(x >= lo) and np.all(x <= hi) and acq.last_cmaes.instance in (0, 1, 2)
        assert acq.compute(x[None, :])[0] >= acq.last_cmaes.value - ACQ_RTOL * abs(acq.last_cmaes.value)
    with pytest.raises(RuntimeError):
        CMAES(EI(model(0.3)), lo[:1], hi[:1])
    with pytest.raises(TypeError):
        CMAES(InformationGain(model(0.3)), lo, hi).maximize()
    calls = []
    r = bayesian_optimization(lambda x: calls.append(1) or _branin(x), lo, hi, num_iterations=5, maximizer="cmaes",
                              model_type="gp", n_candidates=200, rng=np.random.RandomState(7))
    assert len(calls) == 5 == len(r["X"]) and all(np.all(lo <= np.asarray(x)) and np.all(np.asarray(x) <= hi) for x in r["X"])
    with pytest.raises(ValueError):
        bayesian_optimization(_branin, lo, hi, maximizer="cmaes", model_type="blr")


@pytest.mark.gpu
def test_working_size_gpu(gpu_ctx):
    _steps(gpu_ctx, 16, 32, 64, 0 + CO.default_eig_every(16, CO.constants(16, 32)), LOGEI, N=1100, T=20, M=4096, z=None,
           gens=(0, 10, 19))
