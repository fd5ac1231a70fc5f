"""The consumers of V = L^-1 K*^T -- full covariance, cross-covariance, information gain, input gradients -- against the
extended-precision oracle past one tile (tests/vcons_checks.py holds the checks, their shapes and the derivation of every
tolerance).

First the oracle's own additions (cov_oracle.Posterior.covariance / .gradients) are pinned on the CPU: the covariance's
diagonal against `predict`'s variance, its symmetry, and the analytic gradients against central differences of the oracle's
own `predict` taken in long double.  Then every check runs twice: through the interpreter (tests/hipemu) and, -m gpu, on the
MI355X.  V5 (the 128-row tile of cross_cov_kernel and gemm_nt_kernel, taken from 2 x num_cu tiles of candidates per pass on)
is sized from the device's CU count; the interpreter reports one CU, where the same check is three tiles."""
import os
import sys

import numpy as np
import pytest

from robo_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cov_oracle as CO  # noqa: E402
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
    V.drop(ctx)
    ctx.close()
    _lib.use_library(None)


@pytest.fixture(scope="module")
def gpu_ctx():
    _lib.use_library(None)
    if _lib.device_count() < 1:
        pytest.skip("no HIP device")
    ctx = _lib.Context(0)
    yield ctx
    V.drop(ctx)
    ctx.close()


# ---- the oracle's additions ------------------------------------------------------------------------------------------------------
ORACLE_CASES = (("matern52", 40, 3), ("rbf", 33, 4), ("fabolas", 40, 4))


@pytest.mark.parametrize("kind,N,D", ORACLE_CASES)
def test_oracle_covariance(kind, N, D):
    """diag covariance(A) == predict(A)'s variance and covariance(A, A) == covariance(A) up to the order of the long-double
    sums (n eps_L amp: the one is np.sum over V * V, the other a matrix product); covariance(A, B) == covariance(B, A)^T
    exactly (the same products summed in the same order)"""
    c = V.case(kind, N, D, 9, nb=5, seed=7)
    p = c.posterior(L)
    C = p.covariance(c.Xcs)
    tol = N * float(np.finfo(L).eps) * c.kscale
    assert np.max(np.abs(np.diag(C) - p.predict(c.Xcs)[1])) <= tol
    assert np.max(np.abs(p.covariance(c.Xcs, c.Xcs) - C)) <= tol
    S = p.covariance(c.Xcs, c.Zs)
    assert S.shape == (9, 5) and S.dtype == L
    assert np.array_equal(S, p.covariance(c.Zs, c.Xcs).T)
    assert np.array_equal(C, C.T)
    assert C.min() < 0.0                                   # signed, not floored
    p64 = c.posterior(np.float64)
    assert p64.covariance(c.Xcs, c.Zs).dtype == np.float64
    assert np.max(np.abs(p64.covariance(c.Xcs, c.Zs) - S)) <= 1e-9 * c.kscale


@pytest.mark.parametrize("kind,N,D", ORACLE_CASES)
def test_oracle_gradients_against_central_differences(kind, N, D):
    """analytic gradients against (f(xs + h e_d) - f(xs - h e_d)) / 2h of the oracle's own predict, everything in long
    double, h = 1e-7 in SCALED coordinates (inv_sqrt_metric = 1), every column including the fidelity column.  Bound: the
    difference quotient carries h^2 f''' / 6 ~ 1e-14 x (a few hundred: third derivatives of the mean in scaled coordinates)
    and the oracle's own error in f over h: eps_L cond(L) |z| ~ 1e-19 x 1e3 x 30 over 2e-7 ~ 1e-8 at the very worst
    (uncorrelated errors left and right; in practice they cancel) -- 1e-7 of the largest gradient entry, ten orders above a
    missing term."""
    c = V.case(kind, N, D, 9, nb=5, seed=7)
    p = c.posterior(L)
    dm, dv = p.gradients(c.Xcs, np.ones(D))
    assert dm.shape == dv.shape == (9, D) and dm.dtype == L
    h = L(1e-7)
    Xl = c.Xcs.astype(L)
    worst = 0.0
    for d in range(D):
        e = np.zeros(D, dtype=L)
        e[d] = h
        (mp, vp), (mm, vm) = p.predict(Xl + e), p.predict(Xl - e)
        step = ((Xl + e) - (Xl - e))[:, d]
        for got, fd, what in ((dm[:, d], (mp - mm) / step, "mean"), (dv[:, d], (vp - vm) / step, "variance")):
            scale = float(np.max(np.abs(dm if what == "mean" else dv)))
            r = float(np.max(np.abs(got - fd))) / (1e-7 * scale)
            worst = max(worst, r)
            assert r <= 1.0, (kind, d, what, r)
    print("oracle gradients %s: worst error / tolerance %.3g" % (kind, worst))
    # the metric's chain rule: d / d x_d = inv_sqrt_metric_d d / d xs_d, in the instance's precision
    dm2, dv2 = p.gradients(c.Xcs, c.ism)
    assert np.array_equal(dm2, dm * c.ism.astype(L)[None, :]) and np.array_equal(dv2, dv * c.ism.astype(L)[None, :])
    if kind == "fabolas":
        assert c.ism[-1] == 1.0 and np.all(dv[:, -1] != 0.0)


# ---- V1 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N,D", V.FULL_COV_CASES)
def test_full_cov_emu(emu_ctx, kind, N, D):
    V.check_full_cov(emu_ctx, kind, N, D)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,N,D", V.FULL_COV_CASES)
def test_full_cov_gpu(gpu_ctx, kind, N, D):
    V.check_full_cov(gpu_ctx, kind, N, D)


def test_refusals_emu(emu_ctx):
    V.check_refusals(emu_ctx)


@pytest.mark.gpu
def test_refusals_gpu(gpu_ctx):
    V.check_refusals(gpu_ctx)


# ---- V2 ----------------------------------------------------------------------------------------------------------------------------
PRODUCER_KINDS = (("matern52", 3), ("fabolas", 4))


@pytest.mark.parametrize("kind,D", PRODUCER_KINDS)
def test_producers_emu(emu_ctx, kind, D):
    V.check_producers(emu_ctx, kind, D)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,D", PRODUCER_KINDS)
def test_producers_gpu(gpu_ctx, kind, D):
    V.check_producers(gpu_ctx, kind, D)


# ---- V3 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N,D,M,nb", V.CROSS_CASES)
def test_cross_cov_emu(emu_ctx, kind, N, D, M, nb):
    V.check_cross_cov(emu_ctx, kind, N, D, M, nb)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,N,D,M,nb", V.CROSS_CASES)
def test_cross_cov_gpu(gpu_ctx, kind, N, D, M, nb):
    V.check_cross_cov(gpu_ctx, kind, N, D, M, nb)


def test_ig_chunked_emu(emu_ctx):
    V.check_ig_chunked(emu_ctx)


@pytest.mark.gpu
def test_ig_chunked_gpu(gpu_ctx):
    V.check_ig_chunked(gpu_ctx)


# ---- V4 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N,D,M", V.GRAD_CASES)
def test_gradients_emu(emu_ctx, kind, N, D, M):
    V.check_gradients(emu_ctx, kind, N, D, M)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,N,D,M", V.GRAD_CASES)
def test_gradients_gpu(gpu_ctx, kind, N, D, M):
    V.check_gradients(gpu_ctx, kind, N, D, M)


# ---- V5 ----------------------------------------------------------------------------------------------------------------------------
def test_wide_tile_emu(emu_ctx):
    """the interpreter reports ONE compute unit: M = 261 is three tiles, the single pass takes the 128-row tile"""
    V.check_wide_tile(emu_ctx, 1)


@pytest.mark.gpu
def test_wide_tile_gpu(gpu_ctx):
    V.check_wide_tile(gpu_ctx, V.device_cu_count())
