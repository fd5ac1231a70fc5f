"""The gradient of the log marginal likelihood -- robo_gp_grad_loglik, robo_gp_grad_loglik_batch -- against the
extended-precision oracle at the edges of its tiles (tests/grad_checks.py holds the checks, their shapes and the derivation of
every tolerance).

First the oracle's own addition (cov_oracle.Posterior.grad_loglik) is pinned on the CPU, with no device: against central
differences of its own long-double log-likelihood in theta.  Then every check runs twice: through the interpreter
(tests/hipemu) and, -m gpu, on the MI355X.  The oracle of a case is computed once per process and shared by both settings.
G1's N = 770, 1024, 1025 (7, 8, 9 block rows) run on the GPU only, and so does N = 641, which takes 17 s through the
interpreter (N = 640 stays in both).  G4's wide batches are sized from the device's CU count; the interpreter reports one CU,
where the same check is a batch of three."""
import os
import sys

import numpy as np
import pytest

from robo_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cov_oracle as CO  # noqa: E402
import grad_checks as G  # noqa: E402
import vcons_checks as V  # noqa: E402

L = np.longdouble


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
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


# ---- the oracle's addition -------------------------------------------------------------------------------------------------------
ORACLE_CASES = (("matern52", 40, 3), ("rbf", 33, 4), ("fabolas", 40, 4))


def _loglik_long(c, theta):
    """the oracle's log-likelihood as a function of a LONG-DOUBLE theta: exp and the scaling of the rows in long double too (the
    device's fp64 scaling, one rounding of 1e-16, would show in a difference quotient over h = 1e-5 as 1e-11)"""
    theta = np.asarray(theta, dtype=L)
    ism = np.ones(c.D, dtype=L)
    ism[:c.d_in] = np.exp(L(-0.5) * theta[1:1 + c.d_in])
    blr = (np.exp(theta[-3]), np.exp(theta[-2])) if c.fab else (L(1), L(1))
    return CO.Posterior(c.kind, np.exp(theta[0]), np.exp(theta[-1]), c.X.astype(L) * ism[None, :], c.y, c.mean, blr=blr).loglik


@pytest.mark.parametrize("kind,N,D", ORACLE_CASES)
def test_oracle_grad_loglik_against_central_differences(kind, N, D):
    """Posterior.grad_loglik against (ll(theta + h e_p) - ll(theta - h e_p)) / 2h of the oracle's own log-likelihood,
    everything in long double, h = 1e-5; the last entry by the chain rule d / d sigma^2 = (1 / sigma^2) d / d ln sigma^2.
    Bound: the quotient carries h^2 ll''' / 6 = 1.7e-11 ll''' (third derivatives in log-space parameters: up to a few hundred
    times the gradient, in ln sigma^2 most of all) and the oracle's own error in ll over h: eps_L cond(L) |ll| ~ 1e-19 x
    1e3 x 1e2 over 2e-5 ~ 1e-9 at the very worst (uncorrelated errors left and right; in practice they cancel) -- 1e-7 of the
    largest entry (for the last entry: of the largest entry times 1 / sigma^2, the factor its quotient is divided by), seven
    orders above a missing term or a factor 2.  The fp64 twin agrees with it to 1e-9 and is fp64; S_p >= |g_p|."""
    c = G.case(kind, N, D, seed=9)
    theta = c.thetas[0]
    amp, noise, blr, Xs = c.parts(theta)
    o = CO.Posterior(kind, amp, noise, Xs, c.y, c.mean, blr=blr)
    g, S = o.grad_loglik()
    assert g.shape == S.shape == (c.P,) and g.dtype == L and S.dtype == L
    assert np.all(S >= np.abs(g)) and np.all(S > 0)
    # the oracle at the fp64-scaled rows and the all-long-double function agree where the difference quotient starts
    assert abs(_loglik_long(c, theta) - o.loglik) <= 1e-12 * abs(float(o.loglik))
    h = L(1e-5)
    scale = float(np.max(np.abs(g[:-1])))
    worst = 0.0
    for p in range(c.P):
        e = np.zeros(c.P, dtype=L)
        e[p] = h
        tp, tm = theta.astype(L) + e, theta.astype(L) - e
        fd = (_loglik_long(c, tp) - _loglik_long(c, tm)) / (tp[p] - tm[p])
        last = p == c.P - 1
        if last:
            fd = fd / np.exp(L(theta[-1]))
        r = float(abs(g[p] - fd)) / (1e-7 * scale * (1.0 / noise if last else 1.0))
        worst = max(worst, r)
        assert r <= 1.0, (kind, p, float(g[p]), float(fd), r)
    print("oracle grad_loglik %s: worst error / tolerance %.3g" % (kind, worst))
    t = CO.Posterior(kind, amp, noise, Xs, c.y, c.mean, blr=blr, dtype=np.float64)
    g64, S64 = t.grad_loglik()
    assert g64.dtype == np.float64 and S64.dtype == np.float64
    assert np.max(np.abs(g64 - g)) <= 1e-9 * float(np.max(np.abs(g)))


def test_oracle_grad_loglik_matches_fp64_restatement():
    """the twin against oracle.gp_oracle.gp_grad_log_likelihood (unscaled rows, LAPACK): the parameter order of the three
    kinds and the mirrored noise entry are those of the restatement the suite has used so far"""
    from oracle import gp_oracle as O
    for kind, N, D in ORACLE_CASES:
        c = G.case(kind, N, D, seed=9)
        amp, noise, blr, Xs = c.parts(c.thetas[0])
        g64, _ = CO.Posterior(kind, amp, noise, Xs, c.y, c.mean, blr=blr, dtype=np.float64).grad_loglik()
        ref = O.gp_grad_log_likelihood(kind, c.thetas[0], c.X, c.y, c.mean)
        np.testing.assert_allclose(g64, ref, rtol=1e-8, atol=1e-9 * np.max(np.abs(ref)))


def test_rule_restatement():
    """grad_checks.triinv_levels at the figures gradient.hip's rule gives on the 256-CU part"""
    assert 2 * 256 // 2 + 1 == 257 and 2 * 256 // 3 + 1 == 171
    assert G.triinv_levels(300, 257, 256) == [(1, 2, False), (2, 1, False)]
    assert G.triinv_levels(300, 256, 256) == [(1, 2, True), (2, 1, False)]
    assert G.triinv_levels(520, 171, 256) == [(1, 3, False), (2, 2, False), (4, 1, False)]
    assert G.triinv_levels(520, 170, 256) == [(1, 3, True), (2, 2, False), (4, 1, False)]
    assert all(n for _, _, n in G.triinv_levels(4096, 1, 256)) and not all(n for _, _, n in G.triinv_levels(4097, 1, 256))
    assert G.sample_bytes(520, 3, 5) * 171 <= G.WS_DEFAULT


# ---- G1, G2 (and G4's ordinary batch on every shape) ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N,D,mean_offset,smooth", G.G1_CASES_EMU)
def test_block_structure_emu(emu_ctx, kind, N, D, mean_offset, smooth):
    G.check_shape(emu_ctx, kind, N, D, mean_offset, smooth)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,N,D,mean_offset,smooth", G.G1_CASES + G.G1_CASES_GPU)
def test_block_structure_gpu(gpu_ctx, kind, N, D, mean_offset, smooth):
    G.check_shape(gpu_ctx, kind, N, D, mean_offset, smooth)


@pytest.mark.parametrize("kind,N,D,mean_offset,smooth", G.G2_CASES)
def test_dimension_passes_emu(emu_ctx, kind, N, D, mean_offset, smooth):
    G.check_shape(emu_ctx, kind, N, D, mean_offset, smooth)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,N,D,mean_offset,smooth", G.G2_CASES)
def test_dimension_passes_gpu(gpu_ctx, kind, N, D, mean_offset, smooth):
    G.check_shape(gpu_ctx, kind, N, D, mean_offset, smooth)


# ---- G3 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N,D", G.G3_CASES)
def test_special_pairs_emu(emu_ctx, kind, N, D):
    G.check_special(emu_ctx, kind, N, D)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,N,D", G.G3_CASES)
def test_special_pairs_gpu(gpu_ctx, kind, N, D):
    G.check_special(gpu_ctx, kind, N, D)


# ---- G4 ----------------------------------------------------------------------------------------------------------------------------
def test_mixed_batch_emu(emu_ctx):
    G.check_mixed_batch(emu_ctx)


@pytest.mark.gpu
def test_mixed_batch_gpu(gpu_ctx):
    G.check_mixed_batch(gpu_ctx)


@pytest.mark.parametrize("N", G.WIDE_N)
def test_wide_batch_emu(emu_ctx, N):
    """the interpreter reports ONE compute unit: S = 3 and 2, TM = 4 at every level"""
    G.check_wide_batch(emu_ctx, 1, N)


@pytest.mark.gpu
@pytest.mark.parametrize("N", G.WIDE_N)
def test_wide_batch_gpu(gpu_ctx, N):
    G.check_wide_batch(gpu_ctx, V.device_cu_count(), N)


# ---- G5 ----------------------------------------------------------------------------------------------------------------------------
def test_reuse_emu(emu_ctx):
    G.check_reuse(emu_ctx)


@pytest.mark.gpu
def test_reuse_gpu(gpu_ctx):
    G.check_reuse(gpu_ctx)
