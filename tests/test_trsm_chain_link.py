"""The chained solve's link (robo_amd/csrc/trsm_chain.hip): what is fetched ahead of a wait and what is announced when.

Everything is compared bit for bit against the launches (`trsm_chain` = 0), with the helpers and outputs of
tests/test_trsm_chain.py: mean, variance, full covariance, acquisition values, screened (max, argmax, flags).

* Both staging depths, forced.  The interpreter's device has one CU, so under the automatic rule (`trsm_small_deep` = -1: deep
  while the workgroups fit the CUs) it only ever runs the DK = 1 instantiation, which stages L one stage ahead; the DK = 2
  instantiation, which holds a whole block column on chip before it waits for v_j, is the one the headline step runs.
  `trsm_small_deep` = 0 and 1 at N in {257, 513} (3 and 5 block rows, n % 128 = 1), M in {1, 17, 130}, D in {3, 16}, the three
  kernels.
* Stale data must differ from fresh data.  The slots and V are not zeroed between launches and every other repeat re-runs the
  same inputs on the same handle, so a consumer that read the previous call's slot or tile would read the right bits.  Here
  the chained calls on ONE candidate handle alternate between two thetas, A and B (every log length-scale shifted by +0.3),
  with a refit in between, each call compared with the launches' bits for its theta.  N = 300: three block rows is the
  shortest chain in which the last row reads a slot (row 0's) that no hand-off of its own covers.  N = 513.  On the MI355X
  also N = 1300: 11 block rows, with M = 130 nine tiles, 99 workgroups.  D = 16, Matern-5/2; N = 513 with the other two kernels
  as well.  Ten alternations on the MI355X, two on the interpreter.
"""
import numpy as np
import pytest

from robo_amd import _lib

from test_trsm_chain import (KERNELS, _bits, _check_shape, _everything, _inputs, _same, emu_ctx, gpu_ctx)  # noqa: F401

DEEP_NS = (257, 513)
DEEP_MS = (1, 17, 130)
DS = (3, 16)
ALT_M = 130


# ---- both staging depths -------------------------------------------------------------------------------------------------------
def _check_depth(ctx, deep, N, D, kern, Ms):
    ctx.set_tuning("trsm_small_deep", deep)
    try:
        _check_shape(ctx, N, D, kern, Ms=Ms)      # (asserts the chained kernel's name on every chained call)
    finally:
        ctx.set_tuning("trsm_small_deep", None)


@pytest.mark.parametrize("M", DEEP_MS)
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("N", DEEP_NS)
@pytest.mark.parametrize("deep", (0, 1))
def test_bits_at_both_depths_emu(emu_ctx, deep, N, D, kern, M):
    _check_depth(emu_ctx, deep, N, D, kern, (M,))


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("N", DEEP_NS)
@pytest.mark.parametrize("deep", (0, 1))
def test_bits_at_both_depths_gpu(gpu_ctx, deep, N, D, kern):
    _check_depth(gpu_ctx, deep, N, D, kern, DEEP_MS)


# ---- alternating thetas on one handle ------------------------------------------------------------------------------------------
def _check_alternating(ctx, N, kern, alternations, D=16, M=ALT_M):
    X, y, theta_a, Xc = _inputs(N, D, M, kern)
    theta_b = theta_a.copy()
    theta_b[1:1 + D] += 0.3
    thetas = {"A": theta_a, "B": theta_b}
    mean_c, eta = float(np.mean(y)), float(y.min())
    gp = _lib.DeviceGP(ctx, kern, N, X.shape[1])
    cand = _lib.Candidates(ctx, Xc)
    now = {}
    gp.refit = lambda: gp.fit(thetas[now["theta"]], mean_c)      # (_everything refits after a failed screen)
    try:
        gp.set_data(X, y)
        ref = {}
        for name in "AB":
            now["theta"] = name
            gp.refit()
            ref[name] = _everything(ctx, gp, cand, Xc, eta, 0)
        for key in ("mean", "var", "cov", "acq"):                # stale bits would not pass for fresh ones
            assert not _bits(ref["A"][key], ref["B"][key]), key
        for rep in range(alternations):
            for name in "AB":
                now["theta"] = name
                gp.refit()
                _same(ref[name], _everything(ctx, gp, cand, Xc, eta, 1), (kern, N, name, rep))
    finally:
        ctx.set_tuning("trsm_chain", None)
        cand.close()
        gp.close()


ALT_CASES = [(300, "matern52")] + [(513, k) for k in KERNELS]


@pytest.mark.parametrize("N,kern", ALT_CASES)
def test_alternating_thetas_emu(emu_ctx, N, kern):
    _check_alternating(emu_ctx, N, kern, 2, M=17)      # (two tiles, one of them with padding rows: the interpreter's time)


@pytest.mark.gpu
@pytest.mark.parametrize("N,kern", ALT_CASES + [(1300, "matern52")])
def test_alternating_thetas_gpu(gpu_ctx, N, kern):
    _check_alternating(gpu_ctx, N, kern, 10)
