"""The device-resident DIRECT maximiser (robo_amd/csrc/direct.hip, robo_acq_direct / robo_acq_direct_marginal,
ClosedFormAcquisition.direct, maximizers.Direct) against tests/direct_oracle.py.

Every enqueued iteration of the device's trace is replayed by the oracle from the values the device took: the potentially
optimal rectangles and their order, the points, fmin and the best, the counters, the stop and deferral bits, and at the end
the whole store (centres, levels, values: every child of every iteration) -- all bit for bit, no tolerances: every decision
of the rule is a comparison of singly rounded operations.  The VALUES are compared with robo_acq_eval_cand on the same B
rows within ACQ_RTOL (tests/_tol.py), not bit for bit: the eager call is free to take the chained small-batch solve, which
the batch-position invariance does not tie to predict_scaled's bits.  CPU: the interpreter (+ one case under the
contracting build); -m gpu: the MI355X.

The "nothing divisible" stop cannot be reached by a run: the largest non-empty divisible class has K_hi = +inf and is always
potentially optimal, so it needs a store of indivisible rectangles only (3^24 of them in one dimension).  test_to_lmax shows
what can be shown: the rectangle at LMAX is never taken again and the run goes on.
"""
import os
import sys

import numpy as np
import pytest

from robo_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import direct_oracle as DO  # noqa: E402
from _tol import ACQ_RTOL  # noqa: E402
from test_cmaes import _branin, _bump_problem, _models, emu_ctx, gpu_ctx  # noqa: E402,F401

ACQS = (("ei", 0.0, 0.0), ("log_ei", 0.0, 0.0), ("log_ei", 0.0, 9.0), ("pi", 0.0, 0.0), ("lcb", 1.0, 0.0))
LOGEI = (("log_ei", 0.0, 0.0),)


@pytest.fixture(scope="module")
def fma_ctx():
    sys.path.insert(0, os.path.join(HERE, "hipemu"))
    import build_emu
    if not os.path.exists(build_emu.HOST_CLANG) or " fma " not in open("/proc/cpuinfo").read():
        pytest.skip("no host clang++ or no FMA for the contracting interpreter")
    _lib.use_library(build_emu.build_fma())
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()
    _lib.use_library(None)


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def ctx(request):
    return request.getfixturevalue(request.param + "_ctx")


def _replay(r, gps, kind, par, etas, B, eps, max_evals, capacity=0, ctx=None):
    """the whole trace against the oracle -> the oracle (its store is the device's)"""
    tr, D = r.trace, gps[0].dim
    o = DO.Direct(D, B, eps, max_evals, capacity)
    o.start(tr["values"][0, 0])
    assert tr["ran"][0] == 1 and np.all(tr["x"][0] == 0.5)
    stop = 0
    for t in range(1, len(tr["ran"])):
        sel = o.select() if not stop else dict(stop=stop)
        stop = sel["stop"]
        assert (stop == 0) == bool(tr["ran"][t]) and (stop == 0 or int(tr["flags"][t]) & stop), (t, stop)
        if stop:
            continue
        ns = len(sel["x"])
        assert (tr["n_po"][t], tr["n_slots"][t], tr["n_before"][t], tr["evals"][t]) == (len(sel["po"]), ns, sel["n"], sel["n"] + ns)
        assert list(tr["po"][t][:len(sel["po"])]) == sel["po"] and np.all(tr["po"][t][len(sel["po"]):] == -1), t
        assert tr["x"][t][:ns].tobytes() == sel["x"].tobytes() and np.all(tr["x"][t][ns:] == tr["x"][t][0]), t
        assert (tr["fmin"][t], tr["best"][t]) == (sel["fmin"], sel["best"]) and bool(int(tr["flags"][t]) & DO.DEFERRED) >= sel["deferred"]
        assert sel["deferred"] <= bool(r.flags & DO.DEFERRED)
        if ctx is not None:                                  # the values: tolerance route (module docstring)
            cand = _lib.Candidates(ctx, tr["x"][t])
            want = _lib.acq_marginal(gps, kind, par, etas, cand)[0] if len(gps) > 1 else gps[0].acq(kind, par, etas[0], cand)[0]
            cand.close()
            np.testing.assert_allclose(tr["values"][t][:ns], want[:ns], rtol=ACQ_RTOL, atol=0)
        o.divide(sel, tr["values"][t][:ns])
    n = len(o.f)
    best, fmin = o.best()
    assert (r.evals, r.iters) == (n, o.iters) and r.x.tobytes() == o.c[best].tobytes() and r.value == (0.0 if fmin == 0 else -fmin)
    for name, want in (("centres", o.c), ("levels", o.lev), ("f", o.f)):
        assert np.array_equal(tr[name][:n], np.array(want, dtype=np.float64)) and not tr[name][n:].any(), name
    want_stop = stop or (DO.STOP_BUDGET if n >= max_evals else DO.STOP_ITERS)
    assert r.flags & 0xF00 == want_stop, (hex(r.flags), hex(want_stop))
    return o


def _run(ctx, D, batch, acqs=LOGEI, scales=(1.0,), max_evals=400, max_iters=12, eps=1e-4, capacity=0, y_nan=False, eta_off=0.0,
         values=True):
    rs, ogps, gps, y = _models(ctx, 30, D, scales)
    try:
        if y_nan:                                            # a NaN target makes every moment NaN
            y = y.copy()
            y[3] = np.nan
            gps[0].set_data(rs.rand(30, D), y)
            gps[0].fit(np.concatenate([[0.0], np.log(np.full(D, 0.12 * D)), [np.log(1e-2)]]), 0.0)
        for kind, par, off in acqs:
            etas = np.nanmin(y) + off + eta_off - 0.05 * np.arange(len(gps))
            how = dict(batch=batch, eps=eps, capacity=capacity, diagnostics=True)
            r = _lib.direct_marginal(gps, kind, par, etas, max_evals, max_iters, **how)
            o = _replay(r, gps, kind, par, etas, batch, eps, max_evals, capacity, ctx if values and not y_nan else None)
            again = _lib.direct_marginal(gps, kind, par, etas, max_evals, max_iters, **how)             # determinism
            assert all(again.trace[k].tobytes() == r.trace[k].tobytes() for k in r.trace) and again.x.tobytes() == r.x.tobytes()
            if len(gps) == 1:
                one = gps[0].direct(kind, par, etas[0], max_evals, max_iters, **how)
                assert all(one.trace[k].tobytes() == r.trace[k].tobytes() for k in r.trace) and one.flags == r.flags
        return r, o
    finally:
        for g in gps:
            g.close()


@pytest.mark.parametrize("D,mult,acqs", [(1, 1, LOGEI), (2, 2, LOGEI), (3, 1, ACQS), (3, 3, LOGEI), (17, 2, LOGEI), (33, 1, LOGEI)])
def test_every_iteration(ctx, D, mult, acqs):
    r, o = _run(ctx, D, 2 * D * mult, acqs)
    assert r.flags & DO.DEFERRED                             # B = 2 D and its small multiples defer ...
    r, o = _run(ctx, D, 2 * D * 64, LOGEI, values=False)
    assert not r.flags & DO.DEFERRED                         # ... a large batch never does


def test_contracting_build(fma_ctx):
    _run(fma_ctx, 3, 12, ACQS)


def test_marginal(ctx):
    _run(ctx, 3, 12, (("log_ei", 0.0, 0.0), ("ei", 0.01, 0.0)), scales=(1.0, 0.6, 1.7))


def test_store_past_one_workgroup(ctx):
    """1500 rectangles: two workgroups' tables merge; a capacity that launches four gives the same bits"""
    a = _run(ctx, 3, 96, max_evals=1500, max_iters=60, values=False)[0]
    b = _run(ctx, 3, 96, max_evals=1500, max_iters=60, capacity=4000, values=False)[0]
    assert a.evals > 1100 and (a.x.tobytes(), a.value, a.evals, a.iters) == (b.x.tobytes(), b.value, b.evals, b.iters)
    assert all(a.trace[k][:a.evals].tobytes() == b.trace[k][:a.evals].tobytes() for k in ("centres", "levels", "f"))


def test_ties_and_nan(ctx):
    """EI underflows to exactly 0 over the whole box (fmin == 0: equal class minima go to the lowest index, equal w_i to the
    lowest dimension); a NaN target makes every value NaN (f = DBL_MAX everywhere)"""
    r, o = _run(ctx, 3, 12, (("ei", 0.0, 0.0),), eta_off=-100.0)
    assert r.value == 0.0 and not np.any(r.trace["f"]) and r.evals > 30 and np.array_equal(r.x, np.full(3, 0.5))
    r, o = _run(ctx, 2, 8, LOGEI, y_nan=True)
    assert r.flags & _lib.FLAG_NAN and np.all(np.array(o.f) == DO.DBL_MAX) and r.value == -DO.DBL_MAX


def test_to_lmax_and_stops(ctx):
    r, o = _run(ctx, 1, 64, LOGEI, max_evals=4000, max_iters=30, eps=0.0, values=False)
    lev, po = r.trace["levels"][:r.evals, 0], r.trace["po"][1:]
    deep = np.flatnonzero(lev == DO.LMAX)
    assert len(deep) > 0 and r.trace["ran"].all() and r.flags & DO.STOP_ITERS
    assert all(np.sum(po == i) <= DO.LMAX for i in deep)              # taken once per level, never at LMAX
    r, o = _run(ctx, 2, 8, LOGEI, max_evals=20, max_iters=50)
    assert r.flags & DO.STOP_BUDGET and 20 <= r.evals < 28 and r.trace["ran"].sum() - 1 == r.iters < 10
    r, o = _run(ctx, 2, 8, LOGEI, max_iters=0)
    assert r.flags & DO.STOP_ITERS and (r.evals, r.iters) == (1, 0) and np.array_equal(r.x, [0.5, 0.5])
    r, o = _run(ctx, 2, 8, LOGEI, capacity=30, max_iters=30)
    assert r.flags & DO.STOP_CAPACITY and 22 < r.evals <= 30


def test_refusals(ctx, monkeypatch):
    rs, ogps, (g, fresh), y = _models(ctx, 30, 3, (1.0, 1.0))
    unfit, fab = _lib.DeviceGP(ctx, "matern52", 30, 3), _lib.DeviceGP(ctx, "fabolas", 30, 3)
    fab.set_data(rs.rand(30, 3), y)
    fab.fit(np.concatenate([[0.0], np.log(np.full(2, 0.4)), np.log([0.5, 0.8, 1e-2])]), 0.0)
    for bad in (dict(batch=4), dict(batch=7), dict(batch=16386), dict(max_evals=0), dict(max_iters=-1), dict(eps=-1.0),
                dict(eps=np.nan), dict(capacity=-1), dict(capacity=1 << 25), dict(gp=fab)):
        a = dict(dict(gp=g, max_evals=20, max_iters=3, batch=6), **bad)
        with pytest.raises(ValueError):
            a.pop("gp").direct("lcb", 1.0, 0.0, **a)
    monkeypatch.setitem(_lib.ACQ_KINDS, "nothing", 9)
    for call in (lambda: g.direct("nothing", 1.0, 0.0), lambda: _lib.direct_marginal([g, g], "lcb", 1.0, 0.0)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(Exception, match="trained first"):
        unfit.direct("lcb", 1.0, 0.0)
    ctx.set_tuning("ws_bytes", 1024)
    try:
        with pytest.raises(_lib.RoboBadShape):
            g.direct("lcb", 1.0, 0.0)
    finally:
        ctx.set_tuning("ws_bytes", None)
    assert g.direct("lcb", 1.0, 0.0, 20, 3).evals > 1                  # the handle is still usable
    for h in (unfit, fab, g, fresh):
        h.close()


def test_no_worse_than_a_uniform_sweep(ctx):
    X, y, theta, _ = _bump_problem()
    g = _lib.DeviceGP(ctx, "matern52", len(X), 2)
    g.set_data(X, y)
    g.fit(theta, float(np.mean(y)))
    cand = _lib.Candidates(ctx, np.random.RandomState(0).rand(2000, 2))
    try:
        sweep = g.acq("log_ei", 0.0, y.min(), cand, want_values=False)[1]
        r = g.direct("log_ei", 0.0, y.min(), 2000, 150)
        print("DIRECT %.6f at %s after %d values, uniform sweep %.6f" % (r.value, r.x, r.evals, sweep))
        assert r.value >= sweep and r.flags & DO.STOP_BUDGET
    finally:
        cand.close()
        g.close()


def test_classes_and_front_end(ctx):
    import inspect
    from robo_amd.acquisition_functions import EI, InformationGain, LogEI, MarginalizationGPMCMC
    from robo_amd.fmin import bayesian_optimization
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.maximizers import Direct
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
    sig = inspect.signature(Direct.__init__).parameters
    assert [(k, sig[k].default) for k in list(sig)[4:]] == [("n_func_evals", 400), ("n_iters", 200), ("verbose", True),
                                                            ("eps", 1e-4), ("batch", None), ("rng", None)]
    for acq in (EI(model(0.3)), MarginalizationGPMCMC(LogEI(Mix()))):
        x = Direct(acq, lo, hi, n_func_evals=60, verbose=False).maximize()
        assert np.array_equal(x, acq.direct(60)) and np.all(x >= lo) and np.all(x <= hi) and acq.last_direct.evals >= 60
        assert acq.compute(x[None, :])[0] >= acq.last_direct.value - ACQ_RTOL * abs(acq.last_direct.value)
    with pytest.raises(TypeError):
        Direct(InformationGain(model(0.3)), lo, hi).maximize()
    import robo_amd.compat
    robo_amd.compat.install()
    try:
        from robo.maximizers.direct import Direct as Aliased
        assert Aliased is Direct
    finally:
        robo_amd.compat.uninstall()
    calls = []
    r = bayesian_optimization(lambda x: calls.append(1) or _branin(x), lo, hi, num_iterations=6, maximizer="direct",
                              model_type="gp", rng=np.random.RandomState(7))
    assert len(calls) == 6 == len(r["X"]) and all(np.all(lo <= np.asarray(x)) and np.all(np.asarray(x) <= hi) for x in r["X"])
    with pytest.raises(ValueError):
        bayesian_optimization(_branin, lo, hi, maximizer="direct", model_type="blr")
