"""The lean finish of the acquisition screen's dot-form bounds kernel (robo_amd/csrc/screen.hip screen_dot_finish_lean, the
tuning key `acq_screen_lean`, the rule of screen_lean_wanted, robo_cand_last_screen_finish).

CPU: through the interpreter (tests/hipemu) with `acq_screen_min` lowered to 0 and `acq_screen_dot` = 1, as in
tests/test_acq_screen_dot.py, whose case class and bound checks this file uses.  -m gpu: the same checks at the same shapes
on the MI355X.

What is asserted:
  finish      |k~ - k| <= SD_LEAN_EPS amp = 8e-13 amp against a long-double restatement of both covariance functions written
              here.  N = 1, D = 1, metric 1, the training row at 0, mean_c = 0, identity output transform: the kernel's mean is
              then ONE product round(k~ A), A = amp alpha as packed, and A itself is what the full finish returns for the
              candidate equal to the training row (k = 1 to the last bit there), so k~ / amp = mu~ / A up to 2 u.  Candidates
              are float32 numbers, so x^2 is exact and t = 5 x^2 carries one rounding (4e-17 in k).  They cover s = -x of the
              exponential at 0 (the training row), 1e-10 (t = 1e-20), both sides of the first twelve and of eight far odd
              multiples of ln 2 / 2 (the polynomial's interval edges), 708 (2^n turns subnormal) and 750, and 6000 points from
              1e-10 to 750.  The interpreter's rsq is 1 / sqrt to the last bit, the hardware's seed is not, so the _gpu twin
              is the binding one for the square root; the polynomial, which is nearly all of the error, is the same on both.
  bounds      U_c >= the unscreened sweep's value >= L_c for EI, LogEI, PI and LCB kappa = 1 at every candidate, and
              |mu~ - mu_sweep| <= 1e-4 of the delta applied, with acq_screen_lean = 1 and under the rule (-1).  Every N in
              {1, 127, 129, 300}, D in {1, 3, 8, 16, 20} and M in {1, 63, 65, 257} occurs in SHAPES; the cross product is not run.
  edges       a candidate 1e3 and one 1e6 box widths outside the data: k~ finite, >= 0 and below 8e-13, bounds that bracket;
              a NaN and an infinite coordinate: survivors, and the screened call's answer is the unscreened one's.
  identity    (max, argmax, flags) bit-identical between acq_screen_lean = 1, acq_screen_lean = 0, acq_screen_fused_tail = 0
              (with what robo_cand_last_screen reports unchanged; robo_cand_last_screen_finish says that the one-workgroup tail
              ran exactly where the survivors were solved and fit one partial block, never with the key at 0) and acq_screen = 0 at
              SHAPES, at a shape with several hundred survivors (more than one partial block) and at one that takes the
              probe; at the six (kernel, shape) pairs of WITHIN_CAP and at MANY the full finish alone stays within the cap for
              every acquisition -- asserted outright -- and the lean finish keeps at least its survivors, within the cap too;
              at the other shapes some acquisition falls back under either finish and only the answer is compared.
  rule        a nearly singular fit (N = 129, D = 3, ln m = 2, noise 1e-8: sum |alpha| beyond the rule's 1.25e6) runs the full
              finish under the rule, bounds byte-identical to acq_screen_lean = 0, and forced onto the lean finish its bounds
              still bracket; the headline's and config 2's recipe (N = 256 rows) run the lean one, Fabolas has no finish to choose.

Measured (`pytest -s` prints every figure; NOTES.md "The screen's lean finish and folded launches"):
  max |k~ - k| / amp   Matern-5/2 7.807e-13, RBF 7.278e-13 on the interpreter and on the MI355X alike (the full finish: 4.0e-16,
                       1.9e-16): the polynomial's 7.8153e-13 is all of it, and the hardware's rsq seed changes no digit shown;
  max |mu~ - mu_sweep| in units of the delta applied: 9.7e-5 at N = 1, where the lean term is nearly all of delta and the
                       polynomial nearly all of the error, so the ratio approaches 7.82e-13 / 8e-13 of the 1e-4 it is built
                       for and cannot pass it; at most 3.8e-5 at the other SHAPES, 2.0e-5 for the far candidates;
  survivors            the full finish's count at every shape and acquisition (1 - 52 where the screen prunes; 755 and 172 at MANY).
"""
import os
import sys

import numpy as np
import pytest

from robo_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_acq_screen_dot as TD  # noqa: E402

LEAN_EPS = 8e-13                  # SD_LEAN_EPS of screen.hip
MU_RATIO_MAX = 1e-4
KERNELS = ("matern52", "rbf")
ACQS = TD.ACQS
SHAPES = (dict(N=1, D=1, M=63), dict(N=1, D=16, M=257), dict(N=127, D=3, M=65), dict(N=127, D=20, M=1),
          dict(N=129, D=8, M=257), dict(N=129, D=1, M=63), dict(N=300, D=16, M=65), dict(N=300, D=3, M=257),
          dict(N=300, D=20, M=63), dict(N=129, D=16, M=1))
# the (kernel, shape) pairs at which the FULL finish keeps every acquisition within the cap (found on the interpreter, asserted
# outright below on both): they carry the survivor checks; at the others some acquisition falls back under either finish
WITHIN_CAP = {("matern52", "N127-D3-M65"), ("matern52", "N129-D8-M257"), ("rbf", "N129-D8-M257"), ("matern52", "N300-D3-M257"),
              ("rbf", "N300-D16-M65"), ("rbf", "N300-D20-M63")}
MANY = dict(N=256, D=16, M=4099)           # LCB kappa = 2 keeps 755 (three partial blocks); EI with eta - 1 takes the probe
_sid = TD._sid
_bits = TD._bits


def _settings(ctx):
    ctx.set_tuning("acq_screen_min", 0)
    ctx.set_tuning("acq_screen_dot", 1)
    ctx.set_tuning("acq_screen_lean", 1)


@pytest.fixture(scope="module")
def emu_ctx():
    lib_path, rccl_path = TD._emu_env()
    _lib.use_library(lib_path)
    ctx = _lib.Context(0)
    assert "hipemu" in ctx.name
    _settings(ctx)
    yield ctx
    _CACHE.clear()
    ctx.close()
    _lib.use_library(None)


@pytest.fixture(scope="module")
def gpu_ctx():
    _lib.use_library(None)
    if _lib.device_count() < 1:
        pytest.skip("no HIP device")
    ctx = _lib.Context(0)
    _settings(ctx)
    yield ctx
    _CACHE.clear()
    ctx.close()


_CACHE = {}


class _LoneRow(TD._Case):
    """N = 1: the recipe standardises y, which a single value does not survive; its first row with y = 0.7 and mean_c = 0.2"""

    def __init__(self, ctx, D, M, kern):
        self.ctx, self.M = ctx, M
        X, _, self.theta, self.Xc = TD.synthetic(2, D, M, 0)
        self.X, self.y = X[:1], np.array([0.7])
        self.mean_c, self.eta = 0.2, 0.7
        self.gp = _lib.DeviceGP(ctx, kern, 1, D)
        self.gp.set_data(self.X, self.y)
        self.refit()
        self.cand = _lib.Candidates(ctx, self.Xc)
        self.mu = self.gp.predict(self.cand)[0]
        self._values = {}


def _case(ctx, shape, kern):
    key = (id(ctx), shape["N"], shape["D"], shape["M"], kern)
    if key not in _CACHE:
        _CACHE[key] = (_LoneRow(ctx, shape["D"], shape["M"], kern) if shape["N"] == 1 else
                       TD._Case(ctx, shape["N"], shape["D"], shape["M"], kern))
    return _CACHE[key]


def _lean(ctx, value):
    return TD._tuned(ctx, "acq_screen_lean", value, 1)


# ---- 1. the finish's error ------------------------------------------------------------------------------------------------------
LD = np.longdouble
LN2 = LD("0.693147180559945309417232121458176568")


def _targets():
    """values of s = -x, the exponential's argument"""
    odd = np.concatenate([np.arange(1, 25, 2), [101, 333, 1001, 1501, 1999, 2041, 2043, 2163]]).astype(LD) * LN2 / 2
    s = np.concatenate([[LD(1e-10)], odd * (1 - LD(1e-7)), odd, odd * (1 + LD(1e-7)), [LD(707.9), LD(708.0), LD(708.5), LD(750.0)],
                        np.logspace(-10, np.log10(750.0), 3000).astype(LD), np.linspace(0.0, 60.0, 3000).astype(LD)])
    return s


def _check_finish(ctx, kern):
    amp = 1.3
    theta = np.array([np.log(amp), 0.0, np.log(1e-3)])
    s = _targets()
    x = np.sqrt(s * s / 5 if kern == "matern52" else 2 * s).astype(np.float32).astype(np.float64)
    Xc = np.concatenate([[0.0], x])[:, None]
    gp = _lib.DeviceGP(ctx, kern, 1, 1)
    gp.set_data(np.zeros((1, 1)), np.array([1.7]))
    gp.set_output_transform(0.0, 1.0)
    gp.fit(theta, 0.0)
    cand = _lib.Candidates(ctx, Xc)
    try:
        with _lean(ctx, 0):
            up, lo = gp.screen_bounds("lcb", 0.0, 0.0, cand)
            assert cand.screen_finish() == _lib.SCREEN_FINISH_FULL
        A = -(up[0] + lo[0]) / 2                     # amp alpha as packed: k = 1 to the last bit at the training row
        k_full = (-(up + lo) / 2 / A).astype(LD)
        up, lo = gp.screen_bounds("lcb", 0.0, 0.0, cand)
        assert cand.screen_finish() == _lib.SCREEN_FINISH_LEAN and cand.bounds_kernel() == TD.DOT
        k_lean = (-(up + lo) / 2 / A).astype(LD)
    finally:
        cand.close()
        gp.close()
    xl = Xc[:, 0].astype(LD)
    if kern == "matern52":
        sl = np.sqrt(5 * xl * xl)
        k = (1 + sl + sl * sl / 3) * np.exp(-sl)
    else:
        k = np.exp(-xl * xl / 2)
    e_lean, e_full = np.abs(k_lean - k), np.abs(k_full - k)
    i = int(np.argmax(e_lean))
    print("%s: max |k~ - k| / amp lean %.3e (at x = %.6g), full %.3e, A = %.6g" % (kern, float(e_lean[i]), Xc[i, 0],
                                                                                  float(e_full.max()), A))
    assert np.isfinite(A) and A > 0
    assert np.all(np.isfinite(k_lean.astype(np.float64))) and np.all(k_lean >= 0)
    assert float(e_lean.max()) <= LEAN_EPS, (kern, float(e_lean.max()), Xc[i, 0])


@pytest.mark.parametrize("kern", KERNELS)
def test_finish_error_emu(emu_ctx, kern):
    _check_finish(emu_ctx, kern)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNELS)
def test_finish_error_gpu(gpu_ctx, kern):
    _check_finish(gpu_ctx, kern)


# ---- 2. brackets and ratio -----------------------------------------------------------------------------------------------------
def _check_bounds(ctx, c, label):
    for lean, want in ((1, _lib.SCREEN_FINISH_LEAN), (-1, None)):
        with _lean(ctx, lean):
            ratio = TD._mu_ratio(c, "%s, acq_screen_lean = %d" % (label, lean))
            finish = c.cand.screen_finish()
            assert c.cand.bounds_kernel() == TD.DOT and finish == (want or finish), label
            assert finish in (_lib.SCREEN_FINISH_LEAN, _lib.SCREEN_FINISH_FULL)
            assert ratio <= MU_RATIO_MAX, (label, lean, ratio)
            TD._brackets(c, label)


@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_bounds_emu(emu_ctx, shape, kern):
    _check_bounds(emu_ctx, _case(emu_ctx, shape, kern), "%s %s" % (kern, _sid(shape)))


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_bounds_gpu(gpu_ctx, shape, kern):
    _check_bounds(gpu_ctx, _case(gpu_ctx, shape, kern), "%s %s" % (kern, _sid(shape)))


# ---- 3. edges -------------------------------------------------------------------------------------------------------------------
def _check_far(ctx, kern):
    """N = 1 as in the finish's check: k~ itself is read; then a fitted shape whose first two candidates are far outside"""
    theta = np.array([0.0, 0.0, np.log(1e-3)])
    gp = _lib.DeviceGP(ctx, kern, 1, 1)
    gp.set_data(np.zeros((1, 1)), np.array([1.7]))
    gp.set_output_transform(0.0, 1.0)
    gp.fit(theta, 0.0)
    cand = _lib.Candidates(ctx, np.array([[0.0], [1e3], [-1e3], [1e6], [-1e6], [40.0]]))
    try:
        with _lean(ctx, 0):
            up, lo = gp.screen_bounds("lcb", 0.0, 0.0, cand)
        A = -(up[0] + lo[0]) / 2
        up, lo = gp.screen_bounds("lcb", 0.0, 0.0, cand)
        assert cand.screen_finish() == _lib.SCREEN_FINISH_LEAN
    finally:
        cand.close()
        gp.close()
    k = -(up + lo) / 2 / A
    print("%s far candidates: k~ / amp = %s" % (kern, k))
    assert np.all(np.isfinite(up)) and np.all(np.isfinite(lo))
    assert np.all(k[1:] >= 0) and np.all(k[1:] <= LEAN_EPS), k
    c = TD._Case(ctx, 130, 5, 200, kern)
    c.Xc[0], c.Xc[1] = 1e3, -1e6
    c.cand.close()
    c.cand = _lib.Candidates(ctx, c.Xc)
    c.mu = c.gp.predict(c.cand)[0]
    _check_bounds(ctx, c, "%s far candidates" % kern)
    c.close()


def _check_nan_inf(ctx, kern):
    c = TD._Case(ctx, 130, 5, 200, kern)
    c.Xc[5, 2], c.Xc[9, 0] = np.nan, np.inf
    c.cand.close()
    c.cand = _lib.Candidates(ctx, c.Xc)
    for kind, par in ACQS:
        with TD._tuned(ctx, "acq_screen", 0, None):
            off = c.gp.acq(kind, par, c.eta, c.cand, want_values=False)[1:]
        up, lo = c.gp.screen_bounds(kind, par, c.eta, c.cand)
        assert c.cand.screen_finish() == _lib.SCREEN_FINISH_LEAN
        b = np.nanmax(lo)
        assert not (up[5] < b) and not (up[9] < b), (kind, up[5], up[9], b)          # survivors
        c.refit()
        on = c.gp.acq(kind, par, c.eta, c.cand, want_values=False)[1:]
        assert c.cand.last_screen()[0] == c.M
        assert (_bits([on[0]], [off[0]]) or (np.isnan(on[0]) and np.isnan(off[0]))) and on[1:] == off[1:], (kind, on, off)
    c.close()


@pytest.mark.parametrize("kern", KERNELS)
def test_edges_emu(emu_ctx, kern):
    _check_far(emu_ctx, kern)
    _check_nan_inf(emu_ctx, kern)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNELS)
def test_edges_gpu(gpu_ctx, kern):
    _check_far(gpu_ctx, kern)
    _check_nan_inf(gpu_ctx, kern)


# ---- 4. same answer, bit for bit ------------------------------------------------------------------------------------------------
def _argmax_only(ctx, c, kind, par, eta, lean):
    with _lean(ctx, lean):
        c.refit()                                  # every call starts without a back-off
        out = c.gp.acq(kind, par, eta, c.cand, want_values=False)[1:]
        return out, c.cand.last_screen() + (c.cand.screen_tail_fused(),), c.cand.screen_finish()


def _check_same_answer(ctx, c, label, acqs=ACQS, eta_shift=0.0, expect=None, within_cap=False):
    cap = max(1, c.M * 25 // 100)                  # acq_screen_keep_max = 25
    eta = c.eta + eta_shift
    for kind, par in acqs:
        with TD._tuned(ctx, "acq_screen", 0, None):
            off = c.gp.acq(kind, par, eta, c.cand, want_values=False)[1:]
        on1, (n1, kept1, out1, tail1), fin1 = _argmax_only(ctx, c, kind, par, eta, 1)
        on0, (n0, kept0, out0, tail0), fin0 = _argmax_only(ctx, c, kind, par, eta, 0)
        with TD._tuned(ctx, "acq_screen_fused_tail", 0, None):
            on2, (n2, kept2, out2, tail2), _ = _argmax_only(ctx, c, kind, par, eta, 1)
        assert (n2, kept2, out2) == (n1, kept1, out1), (kind, (n2, kept2, out2), (n1, kept1, out1))
        # the one-workgroup tail ran exactly where the survivors were solved and fit one partial block, and never with the key at 0
        solved1 = out1 in (_lib.SCREEN_SCREENED, _lib.SCREEN_PROBE_USED)
        assert tail1 == (solved1 and kept1 <= 256) and not tail2, (kind, tail1, tail2, out1, kept1)
        assert tail0 == (out0 in (_lib.SCREEN_SCREENED, _lib.SCREEN_PROBE_USED) and kept0 <= 256), (kind, tail0, out0, kept0)
        print("%s %s: survivors %d (lean) / %d (full) of %d, outcomes %d / %d" % (label, kind, kept1, kept0, c.M, out1, out0))
        assert n1 == n0 and n0 in (0, c.M) and (n0 > 0 or c.M == 1)
        assert n0 == 0 or (fin1, fin0) == (_lib.SCREEN_FINISH_LEAN, _lib.SCREEN_FINISH_FULL)
        for on in (on1, on0, on2):
            assert _bits([on[0]], [off[0]]) and on[1:] == off[1:], (kind, on, off)
        if within_cap:
            assert n0 == c.M and out0 == out1 == _lib.SCREEN_SCREENED and 1 <= kept0 <= kept1 <= cap, (kind, kept0, kept1, cap, out0)
        if n0 > 0 and out0 == out1:
            assert kept1 >= kept0, (kind, kept1, kept0)
        if n0 > 0 and kept0 <= cap:                         # a condition, not a tolerance
            assert 1 <= kept1 <= cap and out1 != _lib.SCREEN_FELL_BACK, (kind, kept1, kept0, cap)
        if expect:
            expect(kept0, kept1, out0, out1)


@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_same_answer_emu(emu_ctx, shape, kern):
    _check_same_answer(emu_ctx, _case(emu_ctx, shape, kern), "%s %s" % (kern, _sid(shape)),
                       within_cap=(kern, _sid(shape)) in WITHIN_CAP)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_same_answer_gpu(gpu_ctx, shape, kern):
    _check_same_answer(gpu_ctx, _case(gpu_ctx, shape, kern), "%s %s" % (kern, _sid(shape)),
                       within_cap=(kern, _sid(shape)) in WITHIN_CAP)


def _check_many_and_probe(ctx):
    c = _case(ctx, MANY, "matern52")

    def many(kept0, kept1, out0, out1):
        assert out0 == out1 == _lib.SCREEN_SCREENED and 256 < kept0 <= kept1 <= c.M // 4, (kept0, kept1, out0, out1)

    def probe(kept0, kept1, out0, out1):
        assert out0 == out1 == _lib.SCREEN_PROBE_USED and 1 <= kept0 <= c.M // 4, (kept0, kept1, out0, out1)

    _check_same_answer(ctx, c, "several hundred survivors", acqs=(("lcb", 2.0),), expect=many)
    _check_same_answer(ctx, c, "the probe", acqs=(("ei", 0.0),), eta_shift=-1.0, expect=probe)


def test_many_and_probe_emu(emu_ctx):
    _check_many_and_probe(emu_ctx)


@pytest.mark.gpu
def test_many_and_probe_gpu(gpu_ctx):
    _check_many_and_probe(gpu_ctx)


# ---- 5. the rule ----------------------------------------------------------------------------------------------------------------
def _check_rule(ctx):
    s = dict(N=129, D=3, M=257)               # ln m = 2 and noise 1e-8: a nearly singular K, sum |alpha| beyond the rule's limit
    th = np.concatenate([[0.0], np.full(s["D"], 2.0), [np.log(1e-8)]])
    c = TD._Case(ctx, s["N"], s["D"], s["M"], "matern52", theta=th)
    with _lean(ctx, -1):
        rule = [c.gp.screen_bounds(kind, par, c.eta, c.cand) for kind, par in ACQS]
        assert c.cand.screen_finish() == _lib.SCREEN_FINISH_FULL and c.cand.bounds_kernel() == TD.DOT
    with _lean(ctx, 0):
        off = [c.gp.screen_bounds(kind, par, c.eta, c.cand) for kind, par in ACQS]
    for (u1, l1), (u0, l0) in zip(rule, off):
        assert _bits(u1, u0) and _bits(l1, l0)
    TD._mu_ratio(c, "tiny noise, forced lean")            # acq_screen_lean = 1: the lean term carries the bounds
    assert c.cand.screen_finish() == _lib.SCREEN_FINISH_LEAN
    TD._brackets(c, "tiny noise, forced lean")
    c.close()
    with _lean(ctx, -1):
        for name, D in (("headline", 16), ("config 2", 8)):
            c = TD._Case(ctx, 256, D, 130, "matern52")
            c.gp.screen_bounds("ei", 0.0, c.eta, c.cand)
            assert c.cand.screen_finish() == _lib.SCREEN_FINISH_LEAN, name
            c.close()
        c = TD._Case(ctx, 130, 3, 130, "fabolas")
        c.gp.screen_bounds("ei", 0.0, c.eta, c.cand)
        assert c.cand.screen_finish() == _lib.SCREEN_FINISH_NONE and c.cand.bounds_kernel() == TD.DIRECT
        c.close()


def test_rule_emu(emu_ctx):
    _check_rule(emu_ctx)


@pytest.mark.gpu
def test_rule_gpu(gpu_ctx):
    _check_rule(gpu_ctx)
