"""The device-resident differential evolution (robo_amd/csrc/de.hip, robo_acq_de_cand / robo_acq_de_marginal_cand,
ClosedFormAcquisition.de, maximizers.DifferentialEvolution(device=True)) against tests/de_oracle.py.

Every row of the device's trace is replayed by the oracle from the row before, the generation's draws and the trial values
the device took -- indices, F, trial points, masks, accept bits, population, values, best, sum, mean, M2 and code, all bit
for bit: the rule names every operation and rounds each once.  The trial values are robo_acq_eval_cand's on the traced
trial points as one batch, bit for bit.  CPU: the interpreter (+ one case under the contracting build); -m gpu: the MI355X.
"""
import os
import sys

import numpy as np
import pytest

from robo_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import de_oracle as DO  # noqa: E402
from bohamiann_oracle import philox  # noqa: E402
from test_cmaes import _branin, _models, emu_ctx, gpu_ctx  # noqa: E402,F401
from test_direct import fma_ctx  # noqa: E402,F401

RULE = dict(f_lo=0.5, f_hi=1.0, cr=0.7, tol=0.01, atol=0.0)


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def ctx(request):
    return request.getfixturevalue(request.param + "_ctx")


def _same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.where(nan, 0.0, got).tobytes() == np.where(nan, 0.0, want).tobytes()


def _acq(gps, kind, par, etas, cand):
    return _lib.acq_marginal(gps, kind, par, etas, cand) if len(gps) > 1 else gps[0].acq(kind, par, etas[0], cand)


def _replay(res, X, vals, draws, rule):
    """every trace row from the one before -> nothing; the result against the final rows"""
    tr = res.trace
    T1, R, NP, D = tr["pop"].shape
    ends = []
    for r in range(R):
        pop, val, best, code, stats, gens = X[r * NP:(r + 1) * NP], vals[r * NP:(r + 1) * NP], None, 0, None, 0
        for g in range(T1):
            c = {k: v[g, r] for k, v in tr.items()}
            zero = ("trial_values", "accept", "F", "a", "b", "jrand", "cross", "repair") if g == 0 or code else ()
            assert not any(c[k].any() for k in zero), (g, r)
            if code:                                         # stopped: copies of the best point, nothing changes
                assert c["code"] == 3 and _same(c["trial"], np.tile(pop[best], (NP, 1))), (g, r)
            else:
                t = None
                if g > 0:
                    t = DO.trials(pop, best, draws(g - 1, r), rule["f_lo"], rule["f_hi"], rule["cr"])
                    for k, w in zip(("F", "a", "b", "jrand", "trial", "cross", "repair"), t):
                        assert _same(c[k], w), (g, r, k)
                    assert np.all((t[4] >= 0) & (t[4] < 1) | ~t[6]) and np.all((t[4] >= 0) & (t[4] <= 1)), (g, r)
                    gens += 1
                acc, pop, val, best, stats, code = DO.select(pop, val, None if t is None else t[4], c["trial_values"],
                                                             rule["tol"], rule["atol"])
                assert _same(tr["accept"][g, r], acc) and c["code"] == code, (g, r, c["code"], code)
            for k, w in zip(("pop", "values", "best", "sum", "mean", "M2"), (pop, val, best) + stats[:3]):
                assert _same(c[k], w), (g, r, k)
        assert res.generations[r] == gens
        ends.append((val[best], pop[best], stats))
    ok = [r for r in range(R) if not np.isnan(ends[r][0])]
    win = max(ok, key=lambda r: (ends[r][0], -r)) if ok else -1
    assert res.instance == win and _same(res.x, ends[max(win, 0)][1]) and _same(res.value, ends[win][0] if ok else np.nan)
    assert bool(res.flags & _lib.FLAG_FROZEN) == bool(np.any(tr["code"] != 0))
    return ends


def _run(ctx, D, NP, R, kind="log_ei", par=0.0, scales=(1.0,), N=40, T=6, u="draw", X=None, seed=11, values=True, **rule):
    rule = dict(RULE, **rule)
    rs, ogps, gps, y = _models(ctx, N, D, scales)
    etas = y.min() - 0.05 * np.arange(len(gps))
    X = rs.rand(R * NP, D) if X is None else X(rs.rand(R * NP, D))
    cand = _lib.Candidates(ctx, X)
    uu = rs.rand(T, R, 1 + NP * (3 + 2 * D)) if u == "draw" else None
    vals, mx = _acq(gps, kind, par, etas, cand)[:2]
    res = _lib.de_marginal(gps, kind, par, etas, cand, R, NP, T, u=uu, seed=seed, diagnostics=True, **rule)
    draws = (lambda g, r: DO.split_u(uu[g, r], NP, D)) if uu is not None else \
        (lambda g, r: DO.philox_draws(philox, seed, g, r, NP, D))
    ends = _replay(res, X, vals, draws, rule)
    assert np.isnan(mx) or res.value >= mx
    for g in range(1, T + 1 if values else 0):               # the values: robo_acq_eval_cand's on the same batch
        batch = _lib.Candidates(ctx, res.trace["trial"][g].reshape(R * NP, D))
        want = _acq(gps, kind, par, etas, batch)[0].reshape(R, NP)
        batch.close()
        live = res.trace["code"][g] != 3
        assert _same(res.trace["trial_values"][g][live], want[live]), g
    return res, gps, cand, etas, uu, ends


def _close(out):
    out[2].close()
    for h in out[1]:
        h.close()


@pytest.mark.parametrize("D,NP,R,kind", [(1, 4, 1, "log_ei"), (2, 5, 3, "ei"), (3, 64, 2, "log_ei"), (17, 65, 2, "log_ei"),
                                         (5, 257, 1, "pi"), (64, 256, 1, "lcb")])
def test_every_generation(ctx, D, NP, R, kind):
    _close(_run(ctx, D, NP, R, kind, par=1.0 if kind == "lcb" else 0.0))


def test_contracting_build(fma_ctx):
    _close(_run(fma_ctx, 3, 64, 2))


def test_independence(ctx):
    out = _run(ctx, 3, 9, 3, values=False)
    three, gps, cand, etas, u = out[:5]
    for r in range(3):
        one = _lib.Candidates(ctx, cand.points()[r * 9:(r + 1) * 9])
        alone = gps[0].de("log_ei", 0.0, etas[0], one, 1, 9, 6, u=u[:, r:r + 1], diagnostics=True)
        one.close()
        assert all(alone.trace[k][:, 0].tobytes() == three.trace[k][:, r].tobytes() for k in three.trace), r
    _close(out)


def test_philox(ctx):
    out = _run(ctx, 3, 7, 2, u=None)
    other = out[1][0].de("log_ei", 0.0, out[3][0], out[2], 2, 7, 6, seed=12, diagnostics=True)
    assert not np.any(other.trace["F"][1] == out[0].trace["F"][1])
    _close(out)


def test_marginal(ctx):
    _close(_run(ctx, 3, 6, 2, scales=(1.0, 0.6)))
    _close(_run(ctx, 3, 6, 2, kind="ei", par=0.01, scales=(1.0, 0.6, 1.7)))
    out = _run(ctx, 3, 6, 2, values=False)
    a, gps, cand, etas, u = out[:5]
    b = gps[0].de("log_ei", 0.0, etas[0], cand, 2, 6, 6, u=u, diagnostics=True)
    assert all(a.trace[k].tobytes() == b.trace[k].tobytes() for k in a.trace)
    assert (a.value, a.instance, a.flags, a.x.tobytes()) == (b.value, b.instance, b.flags, b.x.tobytes())
    _close(out)


@pytest.mark.parametrize("case", ["identical", "nan_member", "nan_y", "repairs", "tol"])
def test_stops_nan_repair(ctx, case):
    if case == "identical":          # the trials of equal rows are that row: generation 0 converges, later rows copy the best
        out = _run(ctx, 3, 8, 2, X=lambda X: np.tile(X[:1], (16, 1)))
        assert np.all(out[0].trace["code"][:, 0] == [0, 1, 3, 3, 3, 3, 3]) and list(out[0].generations) == [1, 1]
    elif case == "nan_member":       # a NaN start member takes the first trial that has a value
        out = _run(ctx, 3, 8, 1, X=lambda X: np.where(np.arange(8)[:, None] == 1, np.nan, X))
        tr = out[0].trace
        assert np.isnan(tr["values"][0, 0, 1]) and tr["accept"][1, 0, 1] == 1 and not np.isnan(tr["values"][1:]).any()
        assert out[0].flags & _lib.FLAG_NAN
    elif case == "repairs":          # F = 2 throws most mutants out of the box
        out = _run(ctx, 3, 8, 2, f_lo=2.0, f_hi=2.0)
        assert out[0].trace["repair"][1:].mean() > 0.2
    elif case == "tol":              # SciPy's test passes after the first generation, far from its threshold
        out = _run(ctx, 3, 8, 2, tol=1e3)
        assert np.all(out[0].trace["code"][:2, 0] == [0, 1]) and all(2 * e[2][2] <= e[2][3] for e in out[5])
    else:                            # a NaN target makes every moment NaN: nothing to select by
        rs, ogps, gps, y = _models(ctx, 40, 2)
        y[3] = np.nan
        gps[0].set_data(rs.rand(40, 2), y)
        gps[0].fit(np.concatenate([[0.0], np.log(np.full(2, 0.24)), [np.log(1e-2)]]), 0.0)
        X = rs.rand(8, 2)
        cand = _lib.Candidates(ctx, X)
        res = gps[0].de("log_ei", 0.0, 0.0, cand, 1, 8, 3, diagnostics=True)
        _replay(res, X, np.full(8, np.nan), lambda g, r: DO.philox_draws(philox, 0, g, r, 8, 2), RULE)
        assert res.instance == -1 and np.all(res.trace["code"][:, 0] == [0, 2, 3, 3]) and res.flags & _lib.FLAG_NAN
        out = (res, gps, cand)
    _close(out)


def test_refusals(ctx, monkeypatch):
    rs, ogps, (g, fresh), y = _models(ctx, 40, 3, (1.0, 1.0))
    unfit, fab, wide = _lib.DeviceGP(ctx, "matern52", 40, 3), _lib.DeviceGP(ctx, "fabolas", 40, 3), _lib.DeviceGP(ctx, "matern52", 40, 64)
    fab.set_data(rs.rand(40, 3), y)
    fab.fit(np.concatenate([[0.0], np.log(np.full(2, 0.4)), np.log([0.5, 0.8, 1e-2])]), 0.0)
    wide.set_data(rs.rand(40, 64), y)
    wide.fit(np.concatenate([[0.0], np.log(np.full(64, 8.0)), [np.log(1e-2)]]), 0.0)
    cand, big, other = (_lib.Candidates(ctx, rs.rand(m, d)) for m, d in ((16, 3), (260, 64), (16, 2)))
    bad_u = rs.rand(2, 2, 1 + 8 * 9)
    bad_u[1, 1, 5] = 1.0
    for bad in (dict(popsize=3), dict(popsize=1025), dict(n_instances=0), dict(n_instances=65), dict(n_generations=-1),
                dict(gp=wide, cand=big, n_instances=1, popsize=260), dict(n_instances=64, popsize=512), dict(f_lo=-0.1),
                dict(f_lo=0.8, f_hi=0.7), dict(f_hi=2.5), dict(f_lo=np.nan), dict(cr=-0.1), dict(cr=1.1), dict(cr=np.nan),
                dict(tol=-1.0), dict(tol=np.nan), dict(atol=-1.0), dict(atol=np.nan), dict(u=bad_u), dict(u=-bad_u),
                dict(u=bad_u * np.nan), dict(gp=fab)):
        a = dict(dict(gp=g, cand=cand, n_instances=2, popsize=8, n_generations=2), **bad)
        with pytest.raises(ValueError):
            a.pop("gp").de("lcb", 1.0, 0.0, a.pop("cand"), **a)
    monkeypatch.setitem(_lib.ACQ_KINDS, "nothing", 9)                  # the library's own verdict on an unknown kind
    for call in (lambda: g.de("nothing", 1.0, 0.0, cand, 2, 8), lambda: _lib.de_marginal([g, g], "lcb", 1.0, 0.0, cand, 2, 8)):
        with pytest.raises(ValueError):
            call()
    for c, how in ((other, (2, 8)), (cand, (2, 7))):                   # another dim; not R NP rows
        with pytest.raises(_lib.RoboBadShape):
            g.de("lcb", 1.0, 0.0, c, *how)
    with pytest.raises(Exception, match="trained first"):
        unfit.de("lcb", 1.0, 0.0, cand, 2, 8)
    ctx.set_tuning("ws_bytes", 1024)
    try:
        with pytest.raises(_lib.RoboBadShape):
            g.de("lcb", 1.0, 0.0, cand, 2, 8)
    finally:
        ctx.set_tuning("ws_bytes", None)
    assert g.de("lcb", 1.0, 0.0, cand, 2, 8, 2).flags & ~_lib.FLAG_FROZEN == 0     # the handle is still usable
    for h in (cand, big, other, unfit, fab, wide, g, fresh):
        h.close()


def test_class_and_front_end(ctx):
    import inspect
    from robo_amd.acquisition_functions import EI, InformationGain, LogEI, MarginalizationGPMCMC
    from robo_amd.fmin import bayesian_optimization
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.maximizers import DifferentialEvolution
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
    sig = inspect.signature(DifferentialEvolution.__init__).parameters
    assert [(k, sig[k].default) for k in list(sig)[4:]] == [("n_iters", 20), ("rng", None), ("batched", False), ("device", False),
                                                            ("n_instances", 1), ("popsize", None)]
    for acq in (EI(model(0.3)), MarginalizationGPMCMC(LogEI(Mix()))):
        mx = DifferentialEvolution(acq, lo, hi, n_iters=5, rng=np.random.RandomState(5), device=True, n_instances=2)
        x = mx.maximize()
        res = acq.last_de
        assert x.shape == (2,) and np.all(x >= lo) and np.all(x <= hi) and res.instance in (0, 1) and max(res.generations) <= 5
        assert acq.compute(x[None, :])[0] >= res.value - 1e-9 * abs(res.value)
    with pytest.raises(TypeError):
        DifferentialEvolution(InformationGain(model(0.3)), lo, hi, device=True).maximize()
    calls = []
    r = bayesian_optimization(lambda x: calls.append(1) or _branin(x), lo, hi, num_iterations=5, maximizer="device_de",
                              model_type="gp", rng=np.random.RandomState(7))
    assert len(calls) == 5 == len(r["X"]) and all(np.all(lo <= np.asarray(x)) and np.all(np.asarray(x) <= hi) for x in r["X"])
    with pytest.raises(ValueError):
        bayesian_optimization(_branin, lo, hi, maximizer="device_de", model_type="blr")
    from scipy import optimize       # device=False is the host form as before: SciPy on the global NumPy stream
    host = DifferentialEvolution(EI(model(0.3)), lo, hi, n_iters=2)
    np.random.seed(3)
    x = host.maximize()
    np.random.seed(3)
    want = optimize.differential_evolution(lambda p: host._score(p[None, :]), list(zip(lo, hi)), maxiter=2)["x"]
    np.testing.assert_array_equal(x, np.clip(want, lo, hi))


@pytest.mark.gpu
def test_working_size_gpu(gpu_ctx):
    _close(_run(gpu_ctx, 16, 240, 64, N=1100, T=20, u=None))
