"""The single-precision first stage of the acquisition screen (robo_amd/csrc/screen.hip screen_dot_finish_single, the cascade
of acq_sweep_best, the tuning key `acq_screen_single`, robo_cand_last_screen_first).

CPU: through the interpreter (tests/hipemu) with `acq_screen_min` = 0, `acq_screen_dot` = 1 and `acq_screen_lean` = 1, as in
tests/test_acq_screen_lean.py, whose cases and helpers (and those of tests/test_acq_screen_dot.py) this file uses.  -m gpu: the
same checks on the MI355X.  Off the device the bare hardware functions are the C++ library's float sqrt / exp2, which round
correctly: the _gpu twins are the binding ones for the hardware's accuracy figures the bound assumes.

What is asserted:
  finish      |k~ - k| <= SD_SINGLE_EPS amp = 6.3e-7 amp against a long-double restatement of both covariance functions, k~
              finite and >= 0.  The one-row GP of test_acq_screen_lean.py (N = 1, D = 1, `lcb` with kappa = 0, identity output
              transform: the mean is one product k~ A), the bounds read under acq_screen_single = 2.  Grid: that file's
              _targets() and EVERY float of the binade [4, 8) of t = 5 r2 (RBF: of -x = r2 / 2) on the MI355X, every 64th on the
              interpreter: the candidate is sqrt(t / 5) as a double, so the kernel's fp64 t is the float up to 3 ulp of a double
              and rounds to exactly that float.
  brackets    under key 2, EI, LogEI, PI and LCB kappa = 1: U_c >= the unscreened sweep's value >= L_c at every candidate;
              |mu~ - mu_sweep| <= delta / SCREEN_SINGLE_SAFETY at every candidate; every survivor of the fp64 lean bounds
              (key 0) is a survivor of the first stage.  SHAPES: N one off 128 and D at every k-step count (1, 3, 8, 16, 20; 17
              with 200 candidates).
  same answer (max, argmax, flags) bit-identical to the acq_screen = 0 call with the key at 1, 0 and -1, after a refit each, at
              SHAPES and at MANY; outcome, finish and kernel as with key 0 wherever the first stage did not decide; stage 1:
              kept <= min(128, cap) and >= the key-0 count; stage 2: (n, kept, outcome) the key-0 call's.  LCB kappa = 2 on
              MANY (755 survivors) and EI at eta - 1 (the probe) report stage 2 and the outcomes of key 0.
  edges       far candidates: finite bounds, 0 <= k~ <= SD_SINGLE_EPS; a finite candidate beyond the floats' range (1e20): k~ NaN
              or 0, a survivor where NaN; NaN / inf coordinates: survivors; answers equal.
  rule, pause the nearly singular fit of test_acq_screen_lean.py is refused (stage 0, bounds byte-identical to key 0);
              acq_screen_lean = 0 and a Fabolas GP give stage 0; a call made to miss, five times without a refit: stages
              2, 0, 2, 0, 0, every answer the unscreened one's; a refit starts afresh.

Measured (`pytest -s` prints every figure; NOTES.md "A single-precision first stage"):
  max |k~ - k| / amp   MI355X, all 8 388 608 floats of the binade and the targets: Matern-5/2 2.243e-7 = 3.76 x 2^-24, RBF
                       4.616e-8 = 0.77 x 2^-24; interpreter (every 64th float): 1.941e-7 = 3.26 x 2^-24 and 5.029e-8; the bound is
                       6.3e-7 = 10.5 x 2^-24, its derivation's sum 9.4 x 2^-24;
  max |mu~ - mu_sweep| in units of the delta applied: 0.15 (allowed 1 / 1.5), interpreter and MI355X alike;
  stages               key 1, SHAPES and the edge cases: 55 calls decided by the first stage, 20 followed by the fp64 pass; MANY:
                       763 first-stage survivors against 755 (LCB kappa = 2), 4099 against the probe's 172, 2 against 2 (EI).
"""
import os
import sys

import numpy as np
import pytest

from robo_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_acq_screen_dot as TD  # noqa: E402
import test_acq_screen_lean as TL  # noqa: E402

SINGLE_EPS = 6.3e-7               # SD_SINGLE_EPS of screen.hip
SINGLE_SAFETY = 1.5               # SCREEN_SINGLE_SAFETY
KERNELS = ("matern52", "rbf")
ACQS = TD.ACQS
SHAPES = (dict(N=1, D=1, M=63), dict(N=127, D=3, M=65), dict(N=129, D=8, M=257), dict(N=129, D=16, M=1),
          dict(N=300, D=16, M=65), dict(N=300, D=20, M=63), dict(N=257, D=17, M=200))
MANY = TL.MANY
_sid = TD._sid
_bits = TD._bits
LD = np.longdouble


@pytest.fixture(scope="module")
def emu_ctx():
    lib_path, rccl_path = TD._emu_env()
    _lib.use_library(lib_path)
    ctx = _lib.Context(0)
    assert "hipemu" in ctx.name
    TL._settings(ctx)
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
    TL._settings(ctx)
    yield ctx
    _CACHE.clear()
    ctx.close()


_CACHE = {}


def _case(ctx, shape, kern):
    key = (id(ctx), shape["N"], shape["D"], shape["M"], kern)
    if key not in _CACHE:
        _CACHE[key] = (TL._LoneRow(ctx, shape["D"], shape["M"], kern) if shape["N"] == 1 else
                       TD._Case(ctx, shape["N"], shape["D"], shape["M"], kern))
    return _CACHE[key]


def _single(ctx, value):
    return TD._tuned(ctx, "acq_screen_single", value, -1)


# ---- 1. the finish's error ------------------------------------------------------------------------------------------------------
def _binade(stride):
    """the floats of [4, 8), every `stride`-th"""
    bits = np.arange(np.float32(4.0).view(np.uint32), np.float32(8.0).view(np.uint32), stride, dtype=np.uint32)
    return bits.view(np.float32).astype(np.float64)


def _check_finish(ctx, kern, stride):
    amp = 1.3
    theta = np.array([np.log(amp), 0.0, np.log(1e-3)])
    s = TL._targets()
    x = np.sqrt(s * s / 5 if kern == "matern52" else 2 * s).astype(np.float32).astype(np.float64)
    t = _binade(stride)
    xb = np.sqrt(t / 5.0 if kern == "matern52" else 2.0 * t)
    Xc = np.concatenate([[0.0], x, xb])[:, None]
    gp = _lib.DeviceGP(ctx, kern, 1, 1)
    gp.set_data(np.zeros((1, 1)), np.array([1.7]))
    gp.set_output_transform(0.0, 1.0)
    gp.fit(theta, 0.0)
    cand = _lib.Candidates(ctx, Xc)
    try:
        with TL._lean(ctx, 0):
            up, lo = gp.screen_bounds("lcb", 0.0, 0.0, cand)
            assert cand.screen_finish() == _lib.SCREEN_FINISH_FULL
        A = -(up[0] + lo[0]) / 2                     # amp alpha as packed: k = 1 to the last bit at the training row
        with _single(ctx, 2):
            up, lo = gp.screen_bounds("lcb", 0.0, 0.0, cand)
            assert cand.screen_finish() == _lib.SCREEN_FINISH_LEAN and cand.bounds_kernel() == TD.DOT
        k_single = -(up + lo) / 2 / A
        width = float(((up - lo) / 2).max() / A)
    finally:
        cand.close()
        gp.close()
    assert np.isfinite(A) and A > 0
    assert np.all(np.isfinite(k_single)) and np.all(k_single >= 0)
    # delta is the first stage's: SAFETY EPS A and a little more (the lean and the dot terms) -- the bounds read ARE key 2's
    assert width >= SINGLE_SAFETY * SINGLE_EPS
    worst, at = 0.0, 0.0
    for a in range(0, len(Xc), 1 << 20):             # long double in slices: the full binade is 8.4e6 points
        xl = Xc[a:a + (1 << 20), 0].astype(LD)
        if kern == "matern52":
            sl = np.sqrt(5 * xl * xl)
            k = (1 + sl + sl * sl / 3) * np.exp(-sl)
        else:
            k = np.exp(-xl * xl / 2)
        e = np.abs(k_single[a:a + (1 << 20)].astype(LD) - k)
        i = int(np.argmax(e))
        if float(e[i]) > worst:
            worst, at = float(e[i]), float(xl[i])
    print("%s: max |k~ - k| / amp single %.3e = %.2f x 2^-24 (at x = %.9g) over %d points, A = %.6g" %
          (kern, worst, worst * 2.0 ** 24, at, len(Xc), A))
    assert worst <= SINGLE_EPS, (kern, worst, at)


@pytest.mark.parametrize("kern", KERNELS)
def test_finish_error_emu(emu_ctx, kern):
    _check_finish(emu_ctx, kern, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNELS)
def test_finish_error_gpu(gpu_ctx, kern):
    _check_finish(gpu_ctx, kern, 1)


# ---- 2. brackets and nesting ----------------------------------------------------------------------------------------------------
def _survivors(up, lo):
    b = np.nanmax(lo) if not np.all(np.isnan(lo)) else -np.inf
    return ~(up < b)


def _check_bounds(ctx, c, label):
    with _single(ctx, 2):
        up, lo = c.gp.screen_bounds("lcb", 0.0, 0.0, c.cand)
        assert c.cand.bounds_kernel() == TD.DOT and c.cand.screen_finish() == _lib.SCREEN_FINISH_LEAN, label
        assert not np.isnan(up).any() and not np.isnan(lo).any(), label
        err, delta = np.abs(-(up + lo) / 2 - c.mu), (up - lo) / 2
        ratio = float((err / delta).max())
        print("%s: max |mu~ - mu_sweep| = %.3e, in units of delta %.3e (allowed %.3f)" % (label, err.max(), ratio,
                                                                                       1 / SINGLE_SAFETY))
        assert np.all(err <= delta / SINGLE_SAFETY), (label, ratio)
        TD._brackets(c, label)
        first = [c.gp.screen_bounds(kind, par, c.eta, c.cand) for kind, par in ACQS]
    with _single(ctx, 0):
        fp64 = [c.gp.screen_bounds(kind, par, c.eta, c.cand) for kind, par in ACQS]
        assert not _bits(up, c.gp.screen_bounds("lcb", 0.0, 0.0, c.cand)[0]), label      # key 2 returned the first stage's bounds
    for (kind, _), (u1, l1), (u0, l0) in zip(ACQS, first, fp64):
        s1, s0 = _survivors(u1, l1), _survivors(u0, l0)
        print("%s %s: survivors %d (first stage) / %d (fp64 lean) of %d" % (label, kind, s1.sum(), s0.sum(), c.M))
        assert np.all(s1[s0]), (label, kind, int((s0 & ~s1).sum()))


@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_bounds_emu(emu_ctx, shape, kern):
    _check_bounds(emu_ctx, _case(emu_ctx, shape, kern), "%s %s" % (kern, _sid(shape)))


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_bounds_gpu(gpu_ctx, shape, kern):
    _check_bounds(gpu_ctx, _case(gpu_ctx, shape, kern), "%s %s" % (kern, _sid(shape)))


# ---- 3. same answer, bit for bit ------------------------------------------------------------------------------------------------
def _argmax_only(ctx, c, kind, par, eta, key, refit=True):
    with _single(ctx, key):
        if refit:
            c.refit()                              # every call starts without a back-off or a pause
        out = c.gp.acq(kind, par, eta, c.cand, want_values=False)[1:]
        return out, c.cand.last_screen(), c.cand.screen_finish(), c.cand.bounds_kernel(), c.cand.screen_first()


def _check_same_answer(ctx, c, label, acqs=ACQS, eta_shift=0.0, expect=None):
    cap = max(1, c.M * 25 // 100)                  # acq_screen_keep_max = 25
    eta = c.eta + eta_shift
    stages = []
    for kind, par in acqs:
        with TD._tuned(ctx, "acq_screen", 0, None):
            off = c.gp.acq(kind, par, eta, c.cand, want_values=False)[1:]
        on0, scr0, fin0, ran0, first0 = _argmax_only(ctx, c, kind, par, eta, 0)
        assert first0 == (0, 0), (label, kind, first0)
        assert _bits([on0[0]], [off[0]]) and on0[1:] == off[1:], (kind, on0, off)
        for key in (1, -1):
            on, scr, fin, ran, (stage, kept_first) = _argmax_only(ctx, c, kind, par, eta, key)
            print("%s %s key %d: stage %d, first stage kept %d; solved %d of %d (key 0: %d), outcomes %d / %d" %
                  (label, kind, key, stage, kept_first, scr[1], c.M, scr0[1], scr[2], scr0[2]))
            assert _bits([on[0]], [off[0]]) and on[1:] == off[1:], (kind, key, on, off)
            assert stage in (0, 1, 2) and (fin, ran) == (fin0, ran0), (kind, key, stage, fin, ran)
            if scr0[0] == 0:                                   # not a call the screen handles (a lone candidate)
                assert stage == 0 and scr == scr0
            if stage == 0:
                assert kept_first == 0 and scr == scr0, (kind, key, scr, scr0)
            elif stage == 1:
                assert scr[0] == scr0[0] == c.M and scr[2] == _lib.SCREEN_SCREENED, (kind, key, scr)
                assert scr[1] == kept_first and 1 <= kept_first <= min(128, cap) and kept_first >= scr0[1], (kind, key, scr, scr0)
            else:
                assert scr == scr0 and not (1 <= kept_first <= min(128, cap)), (kind, key, scr, scr0, kept_first)
            if key == 1:
                assert stage != 0 or scr0[0] == 0, (kind, stage)          # key 1: wherever the lean finish runs
                stages.append(stage)
            if expect:
                expect(stage, scr, scr0)
    return stages


@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_same_answer_emu(emu_ctx, shape, kern):
    _check_same_answer(emu_ctx, _case(emu_ctx, shape, kern), "%s %s" % (kern, _sid(shape)))


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_same_answer_gpu(gpu_ctx, shape, kern):
    _check_same_answer(gpu_ctx, _case(gpu_ctx, shape, kern), "%s %s" % (kern, _sid(shape)))


def _check_many_and_probe(ctx):
    c = _case(ctx, MANY, "matern52")

    def many(stage, scr, scr0):
        assert stage == 2 and scr == scr0 and scr[2] == _lib.SCREEN_SCREENED and scr[1] > 256, (stage, scr, scr0)

    def probe(stage, scr, scr0):
        assert stage == 2 and scr == scr0 and scr[2] == _lib.SCREEN_PROBE_USED, (stage, scr, scr0)

    _check_same_answer(ctx, c, "several hundred survivors", acqs=(("lcb", 2.0),), expect=many)
    _check_same_answer(ctx, c, "the probe", acqs=(("ei", 0.0),), eta_shift=-1.0, expect=probe)
    # ... and the case the first stage is there for: EI at the incumbent, decided by the first stage alone
    stages = _check_same_answer(ctx, c, "EI at eta", acqs=(("ei", 0.0),))
    assert stages == [1], stages


def test_many_and_probe_emu(emu_ctx):
    _check_many_and_probe(emu_ctx)


@pytest.mark.gpu
def test_many_and_probe_gpu(gpu_ctx):
    _check_many_and_probe(gpu_ctx)


# ---- 4. edges -------------------------------------------------------------------------------------------------------------------
def _check_far(ctx, kern):
    theta = np.array([0.0, 0.0, np.log(1e-3)])
    gp = _lib.DeviceGP(ctx, kern, 1, 1)
    gp.set_data(np.zeros((1, 1)), np.array([1.7]))
    gp.set_output_transform(0.0, 1.0)
    gp.fit(theta, 0.0)
    cand = _lib.Candidates(ctx, np.array([[0.0], [1e3], [-1e3], [1e6], [-1e6], [40.0]]))
    try:
        with TL._lean(ctx, 0):
            up, lo = gp.screen_bounds("lcb", 0.0, 0.0, cand)
        A = -(up[0] + lo[0]) / 2
        with _single(ctx, 2):
            up, lo = gp.screen_bounds("lcb", 0.0, 0.0, cand)
    finally:
        cand.close()
        gp.close()
    k = -(up + lo) / 2 / A
    print("%s far candidates: k~ / amp = %s" % (kern, k))
    assert np.all(np.isfinite(up)) and np.all(np.isfinite(lo))
    assert abs(k[0] - 1) <= SINGLE_EPS and np.all(k[1:] >= 0) and np.all(k[1:] <= SINGLE_EPS), k
    c = TD._Case(ctx, 130, 5, 200, kern)
    c.Xc[0], c.Xc[1] = 1e3, -1e6
    c.cand.close()
    c.cand = _lib.Candidates(ctx, c.Xc)
    c.mu = c.gp.predict(c.cand)[0]
    _check_bounds(ctx, c, "%s far candidates" % kern)
    _check_same_answer(ctx, c, "%s far candidates" % kern)
    c.close()


def _check_beyond_float(ctx, kern):
    """a FINITE candidate whose t lies beyond the floats' range (r2 = 2e41 > 6.8e37): the first stage's k~ is NaN there (inf x 0
    for Matern-5/2) or 0 (RBF) -- never a large number --, a NaN bound makes a survivor, and the answer is the unscreened one's"""
    c = TD._Case(ctx, 130, 5, 200, kern)
    c.Xc[3] = 1e20
    c.cand.close()
    c.cand = _lib.Candidates(ctx, c.Xc)
    with _single(ctx, 2):
        up, lo = c.gp.screen_bounds("lcb", 0.0, 0.0, c.cand)
    with _single(ctx, 0):
        up0, lo0 = c.gp.screen_bounds("lcb", 0.0, 0.0, c.cand)
    assert np.isfinite(up0[3]) and np.isfinite(lo0[3])
    mu, mu0 = -(up[3] + lo[3]) / 2, -(up0[3] + lo0[3]) / 2
    print("%s candidate at 1e20: first-stage mean %r, fp64 mean %r" % (kern, mu, mu0))
    assert np.isnan(mu) or abs(mu - mu0) <= (up[3] - lo[3]) / 2 / SINGLE_SAFETY, (kern, mu, mu0)
    assert np.all(np.isfinite(np.delete(up, 3))) and np.all(np.isfinite(np.delete(lo, 3)))
    for kind, par in ACQS:
        with _single(ctx, 2):
            up, lo = c.gp.screen_bounds(kind, par, c.eta, c.cand)
        assert np.isnan(up[3]) or np.isfinite(up[3]), (kind, up[3])
        assert not np.isnan(up[3]) or not (up[3] < np.nanmax(lo))                    # NaN: a survivor
    _check_same_answer(ctx, c, "%s candidate at 1e20" % kern)
    c.close()


def _check_nan_inf(ctx, kern):
    c = TD._Case(ctx, 130, 5, 200, kern)
    c.Xc[5, 2], c.Xc[9, 0] = np.nan, np.inf
    c.cand.close()
    c.cand = _lib.Candidates(ctx, c.Xc)
    for kind, par in ACQS:
        with TD._tuned(ctx, "acq_screen", 0, None):
            off = c.gp.acq(kind, par, c.eta, c.cand, want_values=False)[1:]
        with _single(ctx, 2):
            up, lo = c.gp.screen_bounds(kind, par, c.eta, c.cand)
        b = np.nanmax(lo)
        assert not (up[5] < b) and not (up[9] < b), (kind, up[5], up[9], b)          # survivors
        on, scr, _, _, (stage, _) = _argmax_only(ctx, c, kind, par, c.eta, 1)
        assert scr[0] == c.M and stage in (1, 2)
        assert (_bits([on[0]], [off[0]]) or (np.isnan(on[0]) and np.isnan(off[0]))) and on[1:] == off[1:], (kind, on, off)
    c.close()


@pytest.mark.parametrize("kern", KERNELS)
def test_edges_emu(emu_ctx, kern):
    _check_far(emu_ctx, kern)
    _check_beyond_float(emu_ctx, kern)
    _check_nan_inf(emu_ctx, kern)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNELS)
def test_edges_gpu(gpu_ctx, kern):
    _check_far(gpu_ctx, kern)
    _check_beyond_float(gpu_ctx, kern)
    _check_nan_inf(gpu_ctx, kern)


# ---- 5. the rule and the pause --------------------------------------------------------------------------------------------------
def _stage_of(c, kind="ei", par=0.0, screened=True):
    """the first stage's report for one call; the call itself went through the screen (else stage 0 would say nothing)"""
    c.gp.acq(kind, par, c.eta, c.cand, want_values=False)
    assert (c.cand.last_screen()[2] != _lib.SCREEN_NOT_ELIGIBLE) == screened, c.cand.last_screen()
    return c.cand.screen_first()[0]


def _check_rule(ctx):
    s = dict(N=129, D=3, M=257)               # ln m = 2 and noise 1e-8: a nearly singular K, sum |alpha| beyond the rule's limit
    th = np.concatenate([[0.0], np.full(s["D"], 2.0), [np.log(1e-8)]])
    c = TD._Case(ctx, s["N"], s["D"], s["M"], "matern52", theta=th)
    with TL._lean(ctx, -1):
        with _single(ctx, -1):
            rule = [c.gp.screen_bounds(kind, par, c.eta, c.cand) for kind, par in ACQS]
            assert _stage_of(c) == 0
        with _single(ctx, 0):
            off = [c.gp.screen_bounds(kind, par, c.eta, c.cand) for kind, par in ACQS]
    for (u1, l1), (u0, l0) in zip(rule, off):
        assert _bits(u1, u0) and _bits(l1, l0)
    # the same fit with the lean finish forced: its own term (about 3e5 prior standard deviations of y) is beyond the rule too
    with _single(ctx, -1):
        c.refit()
        assert _stage_of(c) == 0
    c.close()
    c = TD._Case(ctx, 256, 16, 130, "matern52")
    with _single(ctx, 1):
        assert _stage_of(c) in (1, 2)
        with TL._lean(ctx, 0):
            c.refit()
            assert _stage_of(c) == 0
    with _single(ctx, -1), TL._lean(ctx, 0):
        c.refit()
        assert _stage_of(c) == 0
    c.close()
    c = TD._Case(ctx, 130, 3, 130, "fabolas")
    with _single(ctx, 1):
        assert _stage_of(c) == 0 and c.cand.bounds_kernel() == TD.DIRECT          # (screened, by the direct kernel)
    c.close()


def _check_pause(ctx):
    c = _case(ctx, MANY, "matern52")
    eta = c.eta - 1.0                          # the probe's case: the first stage cannot decide it
    with TD._tuned(ctx, "acq_screen", 0, None):
        off = c.gp.acq("ei", 0.0, eta, c.cand, want_values=False)[1:]
    for round_ in range(2):                    # the second round after a refit: afresh
        stages = []
        for call in range(5 if round_ == 0 else 1):
            on, scr, _, _, (stage, _) = _argmax_only(ctx, c, "ei", 0.0, eta, 1, refit=(call == 0))
            assert _bits([on[0]], [off[0]]) and on[1:] == off[1:], (round_, call, on, off)
            assert scr[2] == _lib.SCREEN_PROBE_USED, (round_, call, scr)
            stages.append(stage)
        assert stages == [2, 0, 2, 0, 0][:len(stages)], (round_, stages)


def test_rule_emu(emu_ctx):
    _check_rule(emu_ctx)


def test_pause_emu(emu_ctx):
    _check_pause(emu_ctx)


@pytest.mark.gpu
def test_rule_gpu(gpu_ctx):
    _check_rule(gpu_ctx)


@pytest.mark.gpu
def test_pause_gpu(gpu_ctx):
    _check_pause(gpu_ctx)
