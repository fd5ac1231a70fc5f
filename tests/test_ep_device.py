"""EP for p_min on the device (robo_ep_joint_min, robo_amd/csrc/ep.hip) against the host restatement
(robo_amd/util/epmgp.py joint_min) and the reference's own outputs (tests/golden/ref_host.npz).

Agreement criterion, every case: all four outputs within rtol 1e-8 and atol 1e-10 max|host array|, and per minimiser the
same number of EP sweeps and the same kill flags as the host (counted by driving epmgp._Sites the way _Sites.run does).
CPU: through the interpreter (tests/hipemu), nb <= 20.  -m gpu: the MI355X at nb = 50 and 64, batches, determinism, and
the reference's fixture replays with the device EP in every InformationGain.update.
"""
import os
import sys

import numpy as np
import pytest

from robo_amd import _lib
from robo_amd.util import epmgp

HERE = os.path.dirname(os.path.abspath(__file__))


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


# ---- helpers ---------------------------------------------------------------------------------------------------------
def host_sweeps(mu, sigma):
    """per minimiser: the sweeps _Sites.run performs, -1 where a cut-off killed the minimiser"""
    mu, sigma = np.asarray(mu, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    n = mu.shape[0]
    out = []
    for k in range(n):
        st = epmgp._Sites(mu, sigma, k)
        others = [l for l in range(n) if l != k]
        sweeps = 0
        for _ in range(50):
            sweeps += 1
            total, stop = 0.0, False
            for idx, l in enumerate(others):
                d = st.refine(idx, l)
                if np.isnan(d):
                    stop = True
                    break
                total += abs(d)
            if stop or abs(total) < 0.001:
                break
        out.append(-1 if st.failed else sweeps)
    return np.array(out)


def assert_agree(dev, host):
    for a, b in zip(dev, host):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape
        np.testing.assert_allclose(a, b, rtol=1e-8, atol=1e-10 * np.max(np.abs(b)))


def check_belief(ctx, mu, sigma):
    """device == host (plain and with derivatives), same sweep counts and kill flags -> device sweeps"""
    host = epmgp.joint_min(mu, sigma, with_derivatives=True)
    logP, dmu, dsig, dmumu, sweeps = _lib.ep_joint_min(ctx, mu[None], sigma[None], True)
    assert_agree((logP[0], dmu[0], dsig[0], dmumu[0]), host)
    np.testing.assert_array_equal(sweeps[0], host_sweeps(mu, sigma))
    plain = epmgp.joint_min_device(mu, sigma, ctx=ctx)
    assert_agree([plain], [epmgp.joint_min(mu, sigma)])
    np.testing.assert_array_equal(plain, logP[0])          # the derivatives do not change log p_min
    return sweeps[0]


def golden_beliefs():
    """the inputs of test_infogain.test_ep_matches_reference_epmgp (n = 3, 8, 20), in the same random order"""
    rs = np.random.RandomState(0)
    out = []
    for n in (3, 8, 20):
        A = rs.randn(n, n)
        sigma = A @ A.T / n + 0.1 * np.eye(n)
        out.append((n, rs.randn(n), sigma))
    return out


def dirac(n):
    mu = np.ones(n) * 1e4
    mu[0] = -1e4
    return mu, np.eye(n) * 1e-3


def near_singular(n, rs):
    """rank-one belief plus a 1e-9 diagonal: every pairwise difference f_l - f_k has a variance of ~2e-9"""
    v = rs.randn(n)
    return rs.randn(n) * 1e-3, np.outer(v, v) + 1e-9 * np.eye(n)


def nan_belief():
    """a covariance whose last row/column is +inf: the first site update puts NaN into V (inf - inf), which the host
    reports as an Exception"""
    s = np.eye(3)
    s[2, :2] = s[:2, 2] = np.inf
    return np.zeros(3), s


def realistic_beliefs(nb, count, seed):
    """posteriors (predict(full_cov=True)) of an oracle GP on Branin at representer points clustered near a minimum:
    highly correlated beliefs, as InformationGain.update meets them"""
    from oracle import gp_oracle as O
    rs = np.random.RandomState(seed)
    lo, hi = np.array([-5.0, 0.0]), np.array([10.0, 15.0])

    def branin(x):
        return (x[:, 1] - 5.1 / (4 * np.pi ** 2) * x[:, 0] ** 2 + 5 / np.pi * x[:, 0] - 6) ** 2 + \
            10 * (1 - 1 / (8 * np.pi)) * np.cos(x[:, 0]) + 10

    out = []
    for i in range(count):
        X = lo + (hi - lo) * rs.rand(12 + i % 7, 2)
        theta = np.array([np.log(50.0), np.log(0.3), np.log(0.5), np.log(1e-2)])
        gp = O.OracleGP("matern52", theta, lower=lo, upper=hi)
        gp.train(X, branin(X))
        centre = np.array([np.pi, 2.275]) + rs.randn(2) * 0.3
        Z = np.clip(centre + rs.randn(nb, 2) * np.array([1.0, 1.5]), lo, hi)
        mu, var = gp.predict(Z, full_cov=True)
        out.append((np.asarray(mu, dtype=np.float64).reshape(-1), np.asarray(var, dtype=np.float64)))
    return out


# ---- CPU (interpreter) -----------------------------------------------------------------------------------------------
def test_reference_beliefs_against_host_and_reference(emu_ctx):
    gold = np.load(os.path.join(HERE, "golden", "ref_host.npz"))
    for n, mu, sigma in golden_beliefs():
        check_belief(emu_ctx, mu, sigma)
        dev = _lib.ep_joint_min(emu_ctx, mu[None], sigma[None], True)
        assert_agree([a[0] for a in dev[:4]], [gold["ep_%d_%d" % (n, i)] for i in range(4)])
        assert_agree([epmgp.joint_min_device(mu, sigma, ctx=emu_ctx)], [gold["ep_%d_plain" % n]])


def test_pins_uniform_and_dirac(emu_ctx):
    """test_infogain.test_pmin_pins through the device: uniform belief -> p ~ 1/n; Dirac -> p_0 == 1 exactly, the other
    minimisers killed by the z < -6 cut-off (log p floored at -500 before the normalisation)"""
    n = 10
    p = np.exp(epmgp.joint_min_device(np.zeros(n), np.eye(n), ctx=emu_ctx))
    assert np.all(np.abs(p - 1.0 / n) < 0.03)
    check_belief(emu_ctx, np.zeros(n), np.eye(n))
    mu, sigma = dirac(n)
    assert np.exp(epmgp.joint_min_device(mu, sigma, ctx=emu_ctx))[0] == 1.0
    sweeps = check_belief(emu_ctx, mu, sigma)
    assert sweeps[0] > 0 and np.all(sweeps[1:] == -1)
    logP = epmgp.joint_min_device(mu, sigma, with_derivatives=True, ctx=emu_ctx)[0]
    assert np.all(logP[1:] == logP[1]) and logP[1] < -499.0


@pytest.mark.parametrize("n", [1, 2])
def test_one_and_two_points(emu_ctx, n):
    rs = np.random.RandomState(n)
    A = rs.randn(n, n)
    check_belief(emu_ctx, rs.randn(n), A @ A.T + 0.1 * np.eye(n))


def test_killed_minimiser(emu_ctx):
    """one point far above the others: its site against the lowest has z < -6, the minimiser is killed (sweeps -1, zero
    derivatives, log p from the -500 floor) while the others converge"""
    rs = np.random.RandomState(3)
    n = 6
    A = rs.randn(n, n)
    sigma = A @ A.T / n + 0.05 * np.eye(n)
    mu = rs.randn(n) * 0.2
    mu[4] = 40.0
    sweeps = check_belief(emu_ctx, mu, sigma)
    assert sweeps[4] == -1 and np.all(np.delete(sweeps, 4) > 0)


def check_near_singular(ctx, mu, sigma):
    """Rank-one beliefs are ill-conditioned for EP itself: the HOST's outputs move by up to 1e-2 (relative) when the
    input is perturbed by one ulp (measured: n = 9, diagonal 1e-9: logP 8.6e-6, dlogPdMu 3.8e-4, dlogPdSigma 1.3e-3,
    dlogPdMudMu 1.0e-2; sweep counts change too), so rtol 1e-8 cannot hold against any implementation that rounds
    differently.  The device must stay inside the host's own one-ulp envelope (3 perturbations, x 4)."""
    host = epmgp.joint_min(mu, sigma, with_derivatives=True)
    dev = [a[0] for a in _lib.ep_joint_min(ctx, mu[None], sigma[None], True)[:4]]

    def rel(a, b):
        return np.max(np.abs(a - b) / (np.abs(b) + 1e-10 * np.max(np.abs(b))))

    env = np.full(4, 1e-8)
    for seed in range(3):
        pert = sigma * (1 + 2.220446049250313e-16 * np.random.RandomState(seed).choice([-1, 0, 1], size=sigma.shape))
        env = np.maximum(env, [rel(a, b) for a, b in zip(epmgp.joint_min(mu, pert, with_derivatives=True), host)])
    got = np.array([rel(a, b) for a, b in zip(dev, host)])
    assert np.all(got <= 4 * env), (got, env)


def test_near_singular_covariance(emu_ctx):
    """rank-one beliefs (plus 1e-9 on the diagonal), check_near_singular.  For sites produced by EP from a positive
    semi-definite belief, I + R^T Sigma R >= I, so the jitter ladder (0 / 1e-10 / 1e-6) of the closed form is not
    climbed from such inputs; the ladder and the LU's singular case are reached only by indefinite inputs"""
    rs = np.random.RandomState(11)
    for n in (4, 9, 17):
        mu, sigma = near_singular(n, rs)
        check_near_singular(emu_ctx, mu, sigma)


def test_nan_in_working_covariance_raises_like_the_host(emu_ctx):
    mu, sigma = nan_belief()
    with pytest.raises(Exception) as host:
        epmgp.joint_min(mu, sigma, with_derivatives=True)
    with pytest.raises(Exception) as dev:
        epmgp.joint_min_device(mu, sigma, with_derivatives=True, ctx=emu_ctx)
    assert str(dev.value) == str(host.value)
    assert type(dev.value) is Exception


def test_bad_arguments(emu_ctx):
    rs = np.random.RandomState(0)
    with pytest.raises(ValueError):
        _lib.ep_joint_min(emu_ctx, rs.randn(1, 65), np.eye(65)[None], True)
    with pytest.raises(ValueError):
        _lib.ep_joint_min(emu_ctx, np.zeros((0, 3)), np.zeros((0, 3, 3)), False)
    from robo_amd.acquisition_functions import InformationGain
    with pytest.raises(ValueError):
        InformationGain(None, np.zeros(2), np.ones(2), Nb=65, ep="device")
    with pytest.raises(ValueError):
        InformationGain(None, np.zeros(2), np.ones(2), ep="gpu")


def test_batch_rows_equal_single_calls(emu_ctx):
    rs = np.random.RandomState(7)
    n = 12
    mus, sigmas = [], []
    for _ in range(3):
        A = rs.randn(n, n)
        mus.append(rs.randn(n))
        sigmas.append(A @ A.T / n + 0.1 * np.eye(n))
    mus[1], sigmas[1] = dirac(n)
    batch = _lib.ep_joint_min(emu_ctx, np.array(mus), np.array(sigmas), True)
    for s in range(3):
        one = _lib.ep_joint_min(emu_ctx, mus[s][None], sigmas[s][None], True)
        for a, b in zip(batch, one):
            np.testing.assert_array_equal(a[s], b[0])
    res = epmgp.joint_min_batch(np.array(mus), np.array(sigmas), True, ctx=emu_ctx)
    for a, b in zip(res, batch):
        np.testing.assert_array_equal(a, b)


def test_information_gain_update_routes_to_the_device(emu_ctx, monkeypatch):
    """InformationGain(ep="device") calls joint_min_device in update(); ep=None follows epmgp.default_backend, read at
    update() time; the default backend is the host"""
    from robo_amd.acquisition_functions import InformationGain
    assert epmgp.default_backend == "host"
    calls = []
    real = epmgp.joint_min_device

    def spy(mu, var, with_derivatives=False, ctx=None):
        calls.append(ctx)
        return real(mu, var, with_derivatives, ctx=emu_ctx)

    monkeypatch.setattr(epmgp, "joint_min_device", spy)

    class Model(object):
        def __init__(self):
            rs = np.random.RandomState(2)
            A = rs.randn(6, 6)
            self.mu, self.var = rs.randn(6), A @ A.T / 6 + 0.1 * np.eye(6)

        def get_noise(self):
            return 1e-3

        def predict(self, X, full_cov=False):
            return self.mu, self.var

    def make(ep):
        ig = InformationGain(Model(), np.zeros(2), np.ones(2), Nb=6, ep=ep)
        ig.sample_representer_points = lambda: (setattr(ig, "zb", np.zeros((6, 2))), setattr(ig, "lmb", np.zeros((6, 1))))
        return ig

    host = make("host")
    host.update(host.model)
    dev = make("device")
    dev.update(dev.model)
    assert len(calls) == 1
    assert_agree([dev.logP.ravel(), dev.dlogPdMu, dev.dlogPdSigma, dev.dlogPdMudMu],
                 [host.logP.ravel(), host.dlogPdMu, host.dlogPdSigma, host.dlogPdMudMu])
    dflt = make(None)
    dflt.update(dflt.model)
    assert len(calls) == 1
    monkeypatch.setattr(epmgp, "default_backend", "device")
    dflt.update(dflt.model)
    assert len(calls) == 2


# ---- GPU (MI355X) ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nb", [50, 64])
def test_gpu_realistic_beliefs(gpu_ctx, nb):
    for mu, sigma in realistic_beliefs(nb, 3, seed=nb):
        check_belief(gpu_ctx, mu, sigma)


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [50, 64])
def test_gpu_edge_cases(gpu_ctx, nb):
    rs = np.random.RandomState(nb)
    n = nb
    p = np.exp(epmgp.joint_min_device(np.zeros(n), np.eye(n), ctx=gpu_ctx))
    assert np.all(np.abs(p - 1.0 / n) < 0.03)
    check_belief(gpu_ctx, np.zeros(n), np.eye(n))
    mu, sigma = dirac(n)
    assert np.exp(epmgp.joint_min_device(mu, sigma, ctx=gpu_ctx))[0] == 1.0
    sweeps = check_belief(gpu_ctx, mu, sigma)
    assert np.all(sweeps[1:] == -1)
    mu, sigma = near_singular(n, rs)
    check_near_singular(gpu_ctx, mu, sigma)
    mu, sigma = nan_belief()
    with pytest.raises(Exception) as dev:
        epmgp.joint_min_device(mu, sigma, with_derivatives=True, ctx=gpu_ctx)
    assert "contains NaN" in str(dev.value)
    with pytest.raises(ValueError):
        _lib.ep_joint_min(gpu_ctx, rs.randn(1, 65), np.eye(65)[None], True)


@pytest.mark.gpu
def test_gpu_batch_of_54_equals_single_calls_and_repeats_bit_for_bit(gpu_ctx):
    beliefs = realistic_beliefs(50, 54, seed=5)
    mus = np.array([b[0] for b in beliefs])
    sigmas = np.array([b[1] for b in beliefs])
    batch = _lib.ep_joint_min(gpu_ctx, mus, sigmas, True)
    again = _lib.ep_joint_min(gpu_ctx, mus, sigmas, True)
    for a, b in zip(batch, again):
        np.testing.assert_array_equal(a, b)
    for s in range(54):
        one = _lib.ep_joint_min(gpu_ctx, mus[s][None], sigmas[s][None], True)
        for a, b in zip(batch, one):
            np.testing.assert_array_equal(a[s], b[0])
    for s in (0, 17, 53):
        host = epmgp.joint_min(mus[s], sigmas[s], with_derivatives=True)
        assert_agree([a[s] for a in batch[:4]], host)
        np.testing.assert_array_equal(batch[4][s], host_sweeps(mus[s], sigmas[s]))


@pytest.fixture
def device_backend(monkeypatch):
    _lib.use_library(None)
    if _lib.device_count() < 1:
        pytest.skip("no HIP device")
    monkeypatch.setattr(epmgp, "default_backend", "device")
    yield


@pytest.mark.gpu
def test_gpu_reference_fixtures_with_device_ep(device_backend):
    """the reference's own choices at every replayed iteration, with every InformationGain.update on the device EP"""
    import ref_checks as R
    calls = []
    real = epmgp.joint_min_device

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    epmgp.joint_min_device = counted
    try:
        R.check_ref_infogain()
        R.check_ref_infogain_cost()
        assert R.check_ref_entropy_search_replay() == 6
        assert R.check_ref_entropy_search_gpmcmc_replay() == 3
        assert R.check_ref_fabolas_replay() == 3
    finally:
        epmgp.joint_min_device = real
    assert len(calls) > 0


@pytest.mark.gpu
def test_gpu_front_ends_with_device_ep(gpu_ctx):
    from robo_amd.fmin import entropy_search, fabolas
    lo, hi = np.array([-5.0, 0.0]), np.array([10.0, 15.0])

    def branin(x):
        x = np.asarray(x).ravel()
        return float((x[1] - 5.1 / (4 * np.pi ** 2) * x[0] ** 2 + 5 / np.pi * x[0] - 6) ** 2 +
                     10 * (1 - 1 / (8 * np.pi)) * np.cos(x[0]) + 10)

    r = entropy_search(branin, lo, hi, num_iterations=4, n_init=2, rng=np.random.RandomState(1), chain_length=20,
                       burnin_steps=20, ep="device")
    assert np.all(r["x_opt"] >= lo) and np.all(r["x_opt"] <= hi)

    def objective(x, s):
        return branin(x * (hi - lo) + lo) / 300.0 + 1e-3, 1.0 + s / 100.0

    r = fabolas(objective, np.zeros(2), np.ones(2), s_min=10, s_max=1000, n_init=2, num_iterations=3,
                subsets=[16, 4], burnin=20, chain_length=10, n_hypers=12, rng=np.random.RandomState(2), ep="device")
    assert np.all(np.asarray(r["x_opt"]) >= 0) and np.all(np.asarray(r["x_opt"]) <= 1)
