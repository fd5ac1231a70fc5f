"""Device-resident multi-start MAP optimisation of the hyper-parameters (robo_amd/csrc/hyperopt.hip,
robo_gp_grad_loglik_batch / robo_gp_optimize_hypers, GaussianProcess(optimizer="device"),
bayesian_optimization(hyper_optimizer="device")) against the fp64 oracle through tests/hyperopt_oracle.py.

Whole trajectories are not compared, for the reason given at the top of tests/test_refine.py: every step of the device's
trace is checked on its own -- F and G against the oracle at the device's own trial point; the trial point, the step
length, the code and the accept bit against the rule applied to the device's own stored doubles.
Every check runs through the interpreter (tests/hipemu) and again, marked gpu, on the MI355X at the same sizes.

Measured on the MI355X (6 starts x 25 iterations, 125 accept decisions per input, none exempt as a tie):
  (90, 3):  max rel F error 1.1e-12, max G error 6.8e-6 (the prior's central-difference reference; 5.9e-4 of its
            tolerance), trial point 1.0e-3 of its tolerance
  (150, 8): max rel F error 1.1e-14, max G error 2.5e-6 (5.9e-5 of its tolerance), trial point 3.9e-4 of its tolerance
  GaussianProcess(optimizer="device") against the host default, nll: (90, 3) 57.18 vs 67.08, (120, 20) 120.21 vs 148.54
The bounds are the issue's, not these figures.
"""
import os
import sys

import numpy as np
import pytest

from robo_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hyperopt_oracle as HO  # noqa: E402
from _tol import LOGLIK_RTOL  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402

GRAD_CASES = (("matern52", 70, 3), ("rbf", 200, 5), ("fabolas", 150, 4), ("matern52", 300, 20), ("matern52", 650, 2))
RULE = dict(history=8, step0=0.5, c1=1e-4, gtol=1e-5)


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


# ---- inputs ----------------------------------------------------------------------------------------------------------
def _grad_inputs(kind, N, D, S=5):
    rs = np.random.RandomState(23)
    X = rs.rand(N, D)
    y = np.sin(3 * X.sum(axis=1)) + 0.1 * rs.randn(N)
    P = O.n_kernel_params(kind, D) + 1
    thetas = 0.3 * rs.randn(S, P)
    thetas[:, 1:P - 1] += np.log(0.3 * D) if kind != "fabolas" else 0.0
    thetas[:, -1] = np.log(1e-2) + 0.2 * rs.randn(S)
    if S >= 3:
        thetas[S // 2, 1] = np.nan
    return X, y, float(y.mean()), thetas


def _sample_bytes(N, D, P):
    """what one sample takes of ws_bytes in robo_gp_grad_loglik_batch (hyperopt.hip hyper_sample_bytes)"""
    npad = (N + 1 + 127) // 128 * 128
    t64 = (N + 63) // 64
    return 8 * (3 * npad * npad + npad * (128 + D) + npad + P * (t64 * (t64 + 1) // 2) + P)


def _sinc_inputs():
    rs = np.random.RandomState(5)
    X = rs.rand(90, 3)
    return X, np.sinc(X * 10 - 5).sum(axis=1)


def _sine_inputs(N=150, D=8, seed=3):
    rs = np.random.RandomState(seed)
    X = rs.rand(N, D)
    return X, np.sin(3 * X.sum(axis=1)) + 0.1 * rs.randn(N)


def _default_prior(P, seed=0):
    from robo_amd.priors import DefaultPrior
    pr = DefaultPrior(P, rng=np.random.RandomState(seed))
    return pr, (1, [pr.ln_prior.mean, pr.ln_prior.sigma, pr.tophat.min, pr.tophat.max, pr.horseshoe.scale])


def _trace_setup(X, y):
    """6 starts: p0, 5 prior draws -- one of them moved outside the tophat (dead), one onto a face of the box"""
    D = X.shape[1]
    P = D + 2
    prior, dev_prior = _default_prior(P)
    p0 = np.concatenate([[np.log(2.0)], np.zeros(D), [np.log(1e-3)]])
    starts = np.vstack([p0[None, :], prior.sample_from_prior(5)])
    lower, upper = np.full(P, -20.0), np.full(P, 20.0)
    lower[2:-1], upper[2:-1] = prior.tophat.min, prior.tophat.max       # length scale 1 keeps +-20: start 2 dies there
    starts[2, 1] = 5.0                       # outside the tophat [-10, 2], inside the box: invalid at the start
    starts[4, 2] = upper[2]                  # on a face of the box
    return prior, dev_prior, lower, upper, starts


# ---- 1. / 2. the batched gradient ------------------------------------------------------------------------------------
def _check_grad_batch(ctx, cases):
    for kind, N, D in cases:
        X, y, mean_c, thetas = _grad_inputs(kind, N, D)
        S, P = thetas.shape
        g = _lib.DeviceGP(ctx, kind, N, D)
        g.set_data(X, y)
        ll, grad, st = g.grad_loglik_batch(thetas, mean_c)
        with pytest.raises(Exception, match="trained first"):
            g.predict(X[:2])                                        # left unfitted
        bad = S // 2
        assert st[bad] == _lib.BAD_ARGUMENT and ll[bad] == -np.inf and np.all(np.isnan(grad[bad]))
        for s in range(S):
            if s == bad:
                continue
            assert st[s] == _lib.OK
            ll1, g1 = g.grad_loglik(thetas[s], mean_c)
            assert ll[s] == ll1, (kind, N, D, s)
            np.testing.assert_array_equal(grad[s], g1, err_msg="%s N=%d D=%d sample %d" % (kind, N, D, s))
            ref = O.gp_grad_log_likelihood(kind, thetas[s], X, y, mean_c)
            np.testing.assert_allclose(ll[s], O.gp_log_likelihood(O.gp_compute(kind, thetas[s], X), y, mean_c),
                                       rtol=LOGLIK_RTOL)
            np.testing.assert_allclose(grad[s], ref, rtol=1e-8, atol=1e-9 * np.max(np.abs(ref)))
        ll2, grad2, st2 = g.grad_loglik_batch(thetas, mean_c)       # repeatable bit for bit
        np.testing.assert_array_equal(ll2, ll)
        np.testing.assert_array_equal(grad2, grad)
        np.testing.assert_array_equal(st2, st)
        lla, ga, sta = g.grad_loglik_batch(thetas[:1], mean_c)      # S = 1
        assert sta[0] == _lib.OK and lla[0] == ll[0]
        np.testing.assert_array_equal(ga[0], grad[0])
        g.close()


def _check_grad_groups(ctx, kind="matern52", N=200, D=3):
    """the same call with ws_bytes lowered so that 5 samples go as 3 + 2: the same bits; not one sample: BAD_SHAPE"""
    X, y, mean_c, thetas = _grad_inputs(kind, N, D)
    g = _lib.DeviceGP(ctx, kind, N, D)
    g.set_data(X, y)
    try:
        ll, grad, st = g.grad_loglik_batch(thetas, mean_c)
        per = _sample_bytes(N, D, thetas.shape[1])
        ctx.set_tuning("ws_bytes", 3 * per + per // 2)
        ll2, grad2, st2 = g.grad_loglik_batch(thetas, mean_c)
        np.testing.assert_array_equal(ll2, ll)
        np.testing.assert_array_equal(grad2, grad)
        np.testing.assert_array_equal(st2, st)
        ctx.set_tuning("ws_bytes", per - 8)
        with pytest.raises(_lib.RoboBadShape):
            g.grad_loglik_batch(thetas, mean_c)
        with pytest.raises(_lib.RoboBadShape):
            g.optimize_hypers(mean_c, None, -20.0, 20.0, thetas[:1], n_iters=1)
        ctx.set_tuning("ws_bytes", per)
        ll3, grad3, _ = g.grad_loglik_batch(thetas, mean_c)        # one sample per group
        np.testing.assert_array_equal(ll3, ll)
        np.testing.assert_array_equal(grad3, grad)
    finally:
        ctx.set_tuning("ws_bytes", None)
        g.close()


# ---- 3. every step of the trace on its own ---------------------------------------------------------------------------
def _check_trace(ctx, X, y, label, T=25, repeat=True):
    N, D = X.shape
    prior, dev_prior, lower, upper, starts = _trace_setup(X, y)
    mean_c = float(y.mean())
    g = _lib.DeviceGP(ctx, "matern52", N, D)
    g.set_data(X, y)
    r = g.optimize_hypers(mean_c, dev_prior, lower, upper, starts, n_iters=T, diagnostics=True, **RULE)
    with pytest.raises(Exception, match="trained first"):
        g.predict(X[:2])                                            # left unfitted
    if repeat:
        r2 = g.optimize_hypers(mean_c, dev_prior, lower, upper, starts, n_iters=T, diagnostics=True, **RULE)
        np.testing.assert_array_equal(r2.trace, r.trace)            # two calls, the same bits
        np.testing.assert_array_equal(r2.theta, r.theta)
    g.close()
    trace = r.trace
    K, P = starts.shape
    assert trace.shape == (T + 1, K, 2 * P + 3)
    np.testing.assert_array_equal(trace[0, :, :P], np.clip(starts, lower, upper))
    assert trace[0, 2, -1] == 3 and r.status[2] == 3                # the start outside the tophat is dead
    assert trace[0, 4, 2] == upper[2]                               # the start on the face
    # F and G of every evaluated entry against the oracle at the device's own trial point
    worst_f = worst_g = worst_p = 0.0
    for t in range(T + 1):
        for k in range(K):
            z, F, G, code = trace[t, k, :P], trace[t, k, P], trace[t, k, P + 1:2 * P + 1], trace[t, k, -1]
            if code == 2:
                continue
            ok = HO.valid("matern52", X, y, mean_c, prior, z)
            assert ok == (code != 3), (t, k, code)
            if not ok:
                continue
            Fo, Go, Gp = HO.objective("matern52", X, y, mean_c, prior, z)
            worst_f = max(worst_f, abs(F - Fo) / abs(Fo))
            np.testing.assert_allclose(F, Fo, rtol=LOGLIK_RTOL)
            tol = 1e-8 * np.abs(Go) + 1e-9 * np.max(np.abs(Go)) + 1e-4 * np.maximum(1.0, np.abs(Gp)) * (Gp != 0.0)
            worst_g = max(worst_g, float(np.max(np.abs(G - (Go + Gp)) / np.maximum(tol, 1e-300))))
            worst_p = max(worst_p, float(np.max(np.abs(G - (Go + Gp)))))
            assert np.all(np.abs(G - (Go + Gp)) <= tol), (t, k, G, Go + Gp)
    rep = HO.replay(trace, lower, upper, RULE["step0"], RULE["c1"], RULE["gtol"], RULE["history"])
    print("%s: max rel F error %.2e, max G error %.2e (%.2e of its tolerance), trial point %.2e of its tolerance, "
          "%d decisions, %d exempt, codes %s, status %s"
          % (label, worst_f, worst_p, worst_g, rep["max_trial_err"], rep["decisions"], rep["exempt"],
             np.unique(trace[:, :, -1], return_counts=True), r.status))
    assert rep["exempt"] <= 0.01 * rep["decisions"]
    assert rep["decisions"] > 2 * T                                 # the live starts did take their steps
    assert np.any(trace[1:, :, -1] == 1) and np.any(trace[1:, :, -1] == 0)
    np.testing.assert_array_equal(r.status, rep["status"])
    np.testing.assert_array_equal(r.final, rep["final"])
    np.testing.assert_array_equal(r.values, rep["values"])          # (NaN == NaN for the dead start)
    best = HO.winner(rep["values"], rep["status"])
    assert r.best == best and r.value == rep["values"][best]
    np.testing.assert_array_equal(r.theta, rep["final"][best])
    live = rep["status"] != 3
    assert np.all(rep["values"][live] >= trace[0, live, P])


# ---- 4. rule edges ---------------------------------------------------------------------------------------------------
def _check_edges(ctx):
    X, y = _sinc_inputs()
    N, D = X.shape
    P = D + 2
    mean_c = float(y.mean())
    prior, dev_prior, lower, upper, starts = _trace_setup(X, y)
    g = _lib.DeviceGP(ctx, "matern52", N, D)
    with pytest.raises(Exception, match="trained first"):          # before set_data: the chain's error
        g.optimize_hypers(mean_c, dev_prior, lower, upper, starts, n_iters=1)
    g.set_data(X, y)
    # n_iters = 0: the best start
    r0 = g.optimize_hypers(mean_c, dev_prior, lower, upper, starts, n_iters=0, diagnostics=True, **RULE)
    assert r0.trace.shape == (1, 6, 2 * P + 3)
    best = HO.winner(r0.values, r0.status)
    assert r0.best == best and r0.value == r0.values[best] == r0.trace[0, best, P]
    np.testing.assert_array_equal(r0.theta, np.clip(starts, lower, upper)[best])
    assert r0.status[2] == 3 and np.isnan(r0.values[2])
    # all starts dead
    dead = np.tile(starts[2], (3, 1))
    rd = g.optimize_hypers(mean_c, dev_prior, lower, upper, dead, n_iters=3, diagnostics=True, **RULE)
    assert rd.best == -1 and np.isnan(rd.value) and np.all(np.isnan(rd.theta)) and np.all(rd.status == 3)
    assert np.all(rd.trace[0, :, -1] == 3) and np.all(rd.trace[1:, :, -1] == 2)
    # history = 1 obeys the rule too
    rule1 = dict(RULE, history=1)
    r1 = g.optimize_hypers(mean_c, dev_prior, lower, upper, starts, n_iters=12, diagnostics=True, **rule1)
    rep = HO.replay(r1.trace, lower, upper, RULE["step0"], RULE["c1"], RULE["gtol"], 1)
    np.testing.assert_array_equal(r1.final, rep["final"])
    np.testing.assert_array_equal(r1.status, rep["status"])
    # a start that is already converged freezes at once: gtol above its gradient
    rc = g.optimize_hypers(mean_c, dev_prior, lower, upper, starts[:1], n_iters=3, diagnostics=True,
                           history=8, step0=0.5, c1=1e-4, gtol=1e6)
    assert rc.status[0] == 1 and rc.trace[0, 0, -1] == 1 and np.all(rc.trace[1:, 0, -1] == 2)
    np.testing.assert_array_equal(rc.theta, starts[0])
    # argument errors
    for bad in (dict(starts=np.tile(starts[0], (65, 1))), dict(history=0), dict(history=17), dict(n_iters=-1),
                dict(lower=upper + 1.0), dict(dev_prior=(3, [0.0] * 5))):
        kw = dict(dev_prior=dev_prior, lower=lower, starts=starts, n_iters=2, history=8)
        kw.update(bad)
        with pytest.raises(ValueError):
            g.optimize_hypers(mean_c, kw["dev_prior"], kw["lower"], upper, kw["starts"], n_iters=kw["n_iters"],
                              history=kw["history"])
    g.close()
    # an invalid trial is rejected, not fatal: duplicate inputs with the noise held on -20 leave K = amp k + 2e-9 I, which
    # stops being numerically positive definite near amp = e^16; targets of size 1e5 pull the amplitude up there
    Xd = np.vstack([X[:40], X[:40]])
    yd = 1e5 * np.concatenate([y[:40], y[:40]])
    g = _lib.DeviceGP(ctx, "matern52", 80, D)
    g.set_data(Xd, yd)
    lo, hi = np.full(P, -20.0), np.full(P, 20.0)
    hi[-1] = -20.0
    st = np.array([[14.0, 0.0, 0.0, 0.0, -20.0], [np.log(2.0), 0.0, 0.0, 0.0, np.log(1e-3)]])
    ri = g.optimize_hypers(float(yd.mean()), None, lo, hi, st, n_iters=10, diagnostics=True, **RULE)
    codes = ri.trace[:, 0, -1]
    print("duplicate inputs: codes of start 0 %s, status %s" % (codes, ri.status))
    # (where exactly K stops being positive definite is a matter of rounding: the verdicts are the device's own here)
    assert np.any(codes == 3), "no invalid trial was produced: the case does not test what it is meant to"
    assert ri.trace[0, 0, -1] == 1 and ri.status[0] != 3
    first = int(np.argmax(codes == 3))
    assert ri.trace[first, 0, P] == -np.inf and np.all(np.isnan(ri.trace[first, 0, P + 1:2 * P + 1]))
    rep = HO.replay(ri.trace, lo, hi, RULE["step0"], RULE["c1"], RULE["gtol"], RULE["history"])
    np.testing.assert_array_equal(ri.status, rep["status"])
    np.testing.assert_array_equal(ri.final, rep["final"])
    assert ri.status[1] != 3 and ri.best >= 0
    g.close()


def _check_shape_change(ctx):
    """one live handle through the state-block shapes (3 starts, history 2) -> (4 starts, history 3) -> the first again:
    every reallocation gives the bits of a handle that never held another shape (N = 22, D = 2, 2 iterations: every array
    of the block is non-empty, and the int tail [npairs | state | pending | err] of 4 starts ends on half a double)"""
    X, y = _sine_inputs(22, 2)
    mean_c = float(y.mean())
    prior, dev_prior = _default_prior(4)
    starts = prior.sample_from_prior(4)
    live, fresh = gps = [_lib.DeviceGP(ctx, "matern52", 22, 2) for _ in range(2)]

    def run(g, k, history):
        return g.optimize_hypers(mean_c, dev_prior, -20.0, 20.0, starts[:k], n_iters=2, diagnostics=True,
                                 **dict(RULE, history=history))

    try:
        for g in gps:
            g.set_data(X, y)
        first, more, again = run(live, 3, 2), run(live, 4, 3), run(live, 3, 2)
        for a, b in ((first, again), (more, run(fresh, 4, 3))):
            assert a.best == b.best
            for p, r in ((a.theta, b.theta), (np.float64(a.value), np.float64(b.value)), (a.final, b.final),
                         (a.values, b.values), (a.status, b.status), (a.trace, b.trace)):
                assert p.tobytes() == r.tobytes()
    finally:
        for g in gps:
            g.close()


def _check_fabolas_priors(ctx, N=150, D=4, T=8):
    """prior kinds 0 and 2 on the Fabolas kernel: F and G of every entry against the oracle, the steps against the rule"""
    from robo_amd.priors import EnvPrior
    X, y = _sine_inputs(N, D, seed=11)
    P = D + 3
    mean_c = float(y.mean())
    env = EnvPrior(P, n_ls=D - 1, n_lr=2, rng=np.random.RandomState(2))
    dev_env = (2, [env.ln_prior.mean, env.ln_prior.sigma, env.tophat.min, env.tophat.max, env.horseshoe.scale,
                   env.n_ls, env.n_lr, env.bayes_lin_prior.mean, env.bayes_lin_prior.sigma])
    p0 = np.concatenate([[np.log(0.5)], np.zeros(D - 1), [np.log(0.5), np.log(0.8)], [np.log(1e-2)]])
    starts = np.vstack([p0[None, :], env.sample_from_prior(2)])
    lower, upper = np.full(P, -20.0), np.full(P, 20.0)
    g = _lib.DeviceGP(ctx, "fabolas", N, D)
    g.set_data(X, y)
    for prior, dev_prior in ((None, None), (env, dev_env)):
        r = g.optimize_hypers(mean_c, dev_prior, lower, upper, starts, n_iters=T, diagnostics=True, **RULE)
        n_checked = 0
        for t in range(T + 1):
            for k in range(starts.shape[0]):
                z, F, G, code = r.trace[t, k, :P], r.trace[t, k, P], r.trace[t, k, P + 1:2 * P + 1], r.trace[t, k, -1]
                if code == 2:
                    continue
                ok = HO.valid("fabolas", X, y, mean_c, prior, z)
                assert ok == (code != 3), (t, k, code)
                if not ok:
                    continue
                Fo, Go, Gp = HO.objective("fabolas", X, y, mean_c, prior, z)
                np.testing.assert_allclose(F, Fo, rtol=LOGLIK_RTOL)
                tol = 1e-8 * np.abs(Go) + 1e-9 * np.max(np.abs(Go)) + 1e-4 * np.maximum(1.0, np.abs(Gp)) * (Gp != 0.0)
                assert np.all(np.abs(G - (Go + Gp)) <= tol), (t, k, G, Go + Gp)
                n_checked += 1
        assert n_checked > T
        rep = HO.replay(r.trace, lower, upper, RULE["step0"], RULE["c1"], RULE["gtol"], RULE["history"])
        np.testing.assert_array_equal(r.status, rep["status"])
        np.testing.assert_array_equal(r.final, rep["final"])
        assert r.best == HO.winner(rep["values"], rep["status"])
    g.close()


# ---- 5. classes and front end ----------------------------------------------------------------------------------------
def _models(X, y, **kw):
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models import GaussianProcess
    from robo_amd.priors import DefaultPrior
    D = X.shape[1]
    out = {}
    for opt in ("host", "device"):
        # amplitude 2 D: the kernel's own first parameter is log(amp / D) = log 2, inside the lognormal prior's support --
        # p0 is a valid point for both optimisers (with log(2 / D) < 0 the host path never leaves its 1e25 plateau)
        kernel = (2.0 * D) * Matern52Kernel(np.ones(D), ndim=D)
        prior = DefaultPrior(len(kernel) + 1, rng=np.random.RandomState(0))
        m = GaussianProcess(kernel, prior=prior, lower=np.zeros(D), upper=np.ones(D), rng=np.random.RandomState(1),
                            optimizer=opt, **kw)
        state = prior.rng.get_state()
        m.train(X, y, do_optimize=True)
        out[opt] = (m, state, prior.rng.get_state())
    return out


def _check_model(ctx, X, y):
    ms = _models(X, y)
    host, s0, s1 = ms["host"]
    assert s0[2] == s1[2] and np.array_equal(s0[1], s1[1])          # the default path draws nothing from the prior
    dev = ms["device"][0]
    mu, var = dev.predict(X[:4])                                    # fitted at the winner by train()
    assert np.all(np.isfinite(mu)) and np.all(var > 0)
    np.testing.assert_array_equal(dev._fitted_theta, dev.hypers)
    nll_h, nll_d = host.nll(host.hypers), dev.nll(dev.hypers)
    print("N=%d D=%d: nll host %.6f device %.6f" % (X.shape[0], X.shape[1], nll_h, nll_d))
    assert nll_d <= nll_h + 1e-3 * abs(nll_h)


def _check_front_end(ctx):
    from robo_amd.fmin import bayesian_optimization
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models import GaussianProcess
    from robo_amd.priors import BasePrior

    class Flat(BasePrior):
        def lnprob(self, theta):
            return 0.0

    with pytest.raises(ValueError, match="optimizer='host'"):
        GaussianProcess(2.0 * Matern52Kernel(np.ones(2), ndim=2), prior=Flat(), optimizer="device")
    with pytest.raises(ValueError):
        GaussianProcess(2.0 * Matern52Kernel(np.ones(2), ndim=2), optimizer="gpu")

    def branin(x):
        a, b, c, r, s, t = 1.0, 5.1 / (4 * np.pi ** 2), 5.0 / np.pi, 6.0, 10.0, 1.0 / (8 * np.pi)
        return a * (x[1] - b * x[0] ** 2 + c * x[0] - r) ** 2 + s * (1 - t) * np.cos(x[0]) + s

    lower, upper = np.array([-5.0, 0.0]), np.array([10.0, 15.0])
    with pytest.raises(ValueError):
        bayesian_optimization(branin, lower, upper, num_iterations=4, model_type="gp_mcmc", hyper_optimizer="device",
                              rng=np.random.RandomState(3))
    res = bayesian_optimization(branin, lower, upper, num_iterations=6, n_init=3, model_type="gp", n_candidates=50,
                                hyper_optimizer="device", n_restarts=3, rng=np.random.RandomState(3))
    assert len(res["y"]) == 6 and np.all(np.isfinite(res["y"]))
    assert np.all(np.asarray(res["x_opt"]) >= lower) and np.all(np.asarray(res["x_opt"]) <= upper)


# ---- the tests: interpreter, then the MI355X -------------------------------------------------------------------------
@pytest.mark.parametrize("case", GRAD_CASES, ids=lambda c: "%s-%d-%d" % c)
def test_grad_batch(emu_ctx, case):
    _check_grad_batch(emu_ctx, (case,))


@pytest.mark.gpu
@pytest.mark.parametrize("case", GRAD_CASES, ids=lambda c: "%s-%d-%d" % c)
def test_grad_batch_gpu(gpu_ctx, case):
    _check_grad_batch(gpu_ctx, (case,))


def test_grad_batch_groups(emu_ctx):
    _check_grad_groups(emu_ctx)


@pytest.mark.gpu
def test_grad_batch_groups_gpu(gpu_ctx):
    _check_grad_groups(gpu_ctx)


def test_trace_sinc(emu_ctx):
    _check_trace(emu_ctx, *_sinc_inputs(), label="(90, 3)")


def test_trace_sine(emu_ctx):
    _check_trace(emu_ctx, *_sine_inputs(), label="(150, 8)", repeat=False)    # (the second call is interpreter time)


@pytest.mark.gpu
def test_trace_sinc_gpu(gpu_ctx):
    _check_trace(gpu_ctx, *_sinc_inputs(), label="(90, 3)")


@pytest.mark.gpu
def test_trace_sine_gpu(gpu_ctx):
    _check_trace(gpu_ctx, *_sine_inputs(), label="(150, 8)")


def test_rule_edges(emu_ctx):
    _check_edges(emu_ctx)
    _check_shape_change(emu_ctx)


@pytest.mark.gpu
def test_rule_edges_gpu(gpu_ctx):
    _check_edges(gpu_ctx)
    _check_shape_change(gpu_ctx)


def test_fabolas_priors(emu_ctx):
    _check_fabolas_priors(emu_ctx)


@pytest.mark.gpu
def test_fabolas_priors_gpu(gpu_ctx):
    _check_fabolas_priors(gpu_ctx)


def test_model_sinc(emu_ctx):
    _check_model(emu_ctx, *_sinc_inputs())


def test_model_wide(emu_ctx):
    _check_model(emu_ctx, *_sine_inputs(120, 20, seed=3))


@pytest.mark.gpu
def test_model_sinc_gpu(gpu_ctx):
    _check_model(gpu_ctx, *_sinc_inputs())


@pytest.mark.gpu
def test_model_wide_gpu(gpu_ctx):
    _check_model(gpu_ctx, *_sine_inputs(120, 20, seed=3))


def test_front_end(emu_ctx):
    _check_front_end(emu_ctx)


@pytest.mark.gpu
def test_front_end_gpu(gpu_ctx):
    _check_front_end(gpu_ctx)
