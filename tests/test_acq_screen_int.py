"""The integer form of the acquisition screen's first stage (robo_amd/csrc/screen.hip screen_bounds_dot_int_kernel, common.h
mfma_i8, the tuning key `acq_screen_int`, robo_cand_last_screen_form).

CPU: through the interpreter (tests/hipemu), settings and helpers of tests/test_acq_screen_single.py.  -m gpu: the same checks on
the MI355X.  The bounds are read under `acq_screen_single` = 2 with `acq_screen_int` = 1 unless a test says otherwise.

The pair harness.  Two training rows +-h A (A an integer vector whose largest entry is GRID / 2, so that the rows' extent H and
the grid step h = 2 H / GRID are known), y = (1.7, 0.3), identity output transform, `lcb` with kappa = 0: the mean is
A1 k(c, x1) + A2 k(c, x2).  A1, A2 come from the fp64 pass with the full finish at the two rows themselves (a 2 x 2 system);
the expected mean from a long-double restatement of both covariance functions.

What is asserted (E1 = 6.3e-7, the float finish's bound; E4 = c2 2^20 h^2, the dropped level S4 and the offset that replaces
the clamp; c1, c2 = 0.63, 5/6 for Matern-5/2 and 0.61, 1/2 for RBF -- screen.hip "The integer form"):
  exact       candidates ON the grid, asymmetric, digits at -128 and 127 in every dimension and every position, all corners
              +-GRID:  |mu~ - mu| <= (|A1| + |A2|) (E1 + E4): the grid term is zero.  D = 1, 3, 8, 16.
  bound       random off-grid candidates in the +-2 H box, every coordinate at +-H and +-2 H:
              |mu~ - mu| <= (|A1| + |A2|) (E1 + E4 + c1 sqrt(D) h).
  edges       N in 1, 17, 129, 257; M in 1, 63, 65, 4099; D in 1, 3, 8, 16: the form is the integer one,
              |mu~ - mu_sweep| <= delta / 1.5, U >= value >= L for the four acquisitions, the fp64 pass's survivors are among
              the first stage's.  D = 17: the fp64-MFMA form.
  answers     N = 256, M = 4099, EI, LogEI, PI, LCB: (max, argmax, flags) the unscreened call's and the key-0 call's bits; with
              candidates at 1e20, +-inf, NaN and one grid step outside the range: they survive, same answer; a call made to
              miss five times: stages 2, 0, 2, 0, 0 as with the key at 0.
  rule        a fit whose extent makes the grid's term exceed SCREEN_SINGLE_MAX keeps the fp64-MFMA first stage under the
              rule and takes the integer form under key 1; a one-row fit (no extent) and D = 8 take it under key 1 only,
              D = 16 under the rule.

Measured (`pytest -s` prints every figure; NOTES.md "The first stage on exact int8 products"), interpreter and MI355X alike to
the digits given: on the grid max |mu~ - mu| / (|A1| + |A2|) = 1.3e-7 (Matern-5/2, D = 16; allowed 6.33e-7), 3.4e-8 (RBF); off
it 1.0e-7 (allowed 7.84e-7, of which the grid's term is 1.51e-7).  N = 256, M = 4099: 2, 2, 29, 70 survivors for EI, LogEI, PI,
LCB with either form.
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
import test_acq_screen_single as TS  # noqa: E402

E1 = TS.SINGLE_EPS
SAFETY = TS.SINGLE_SAFETY
GRID, AMAX = 8355000, 8355711          # SD_INT_GRID, SD_INT_AMAX of screen.hip
FORM_FP64, FORM_INT8 = 0, 1            # ROBO_SCREEN_FORM_*
C1 = {"matern52": 0.63, "rbf": 0.61}
C2 = {"matern52": 5.0 / 6.0, "rbf": 0.5}
KERNELS = TS.KERNELS
ACQS = TD.ACQS
LD = np.longdouble
EDGES = (dict(N=1, D=1, M=63), dict(N=17, D=3, M=4099), dict(N=129, D=8, M=65), dict(N=257, D=16, M=1))
MANY = TL.MANY
_sid, _bits = TD._sid, TD._bits


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


def _int(ctx, value):
    return TD._tuned(ctx, "acq_screen_int", value, -1)


def _cov(kern, r2):
    if kern == "matern52":
        s = np.sqrt(5 * r2)
        return (1 + s + s * s / 3) * np.exp(-s)
    return np.exp(-r2 / 2)


# ---- 1. the pair harness: exactness on the grid, the bound off it ----------------------------------------------------------------
def _row_digits(D):
    """the first row's integer coordinates: GRID / 2 in dimension 0 (the extent), lower digits at the ends elsewhere, no two alike"""
    A = np.zeros(D, dtype=np.int64)
    A[0] = GRID // 2
    ends = (-128, 127)
    for d in range(1, D):
        A[d] = (7 * d - 60) * 65536 + ends[d & 1] * 256 + ends[(d >> 1) & 1] + (d % 3)
    assert np.all(np.abs(A) <= GRID // 2)
    return A


def _pair(ctx, kern, D, Bs, off_grid=None):
    """-> (mu~ of the integer first stage, exact mu in long double, |A1| + |A2|, h) for candidates h Bs (+ off_grid)"""
    H = 0.25
    h = 2.0 * H / GRID
    A = _row_digits(D)
    X = np.stack([h * A, -(h * A)])
    Xc = h * np.asarray(Bs, dtype=np.float64) + (0.0 if off_grid is None else off_grid)
    Xc = np.concatenate([X, Xc])
    amp = 1.3
    theta = np.concatenate([[np.log(amp)], np.zeros(D), [np.log(1e-3)]])
    gp = _lib.DeviceGP(ctx, kern, 2, D)
    gp.set_data(X, np.array([1.7, 0.3]))
    gp.set_output_transform(0.0, 1.0)
    gp.fit(theta, 0.0)
    cand = _lib.Candidates(ctx, Xc)
    try:
        with TL._lean(ctx, 0), TS._single(ctx, 0):
            up, lo = gp.screen_bounds("lcb", 0.0, 0.0, cand)
        full = -(up + lo) / 2
        with TS._single(ctx, 2), _int(ctx, 1):
            up, lo = gp.screen_bounds("lcb", 0.0, 0.0, cand)
            form, step = cand.screen_form()
            assert cand.bounds_kernel() == TD.DOT and cand.screen_finish() == _lib.SCREEN_FINISH_LEAN
        assert form == FORM_INT8 and abs(step / h - 1) < 1e-12, (form, step, h)
    finally:
        cand.close()
        gp.close()
    assert np.all(np.isfinite(up)) and np.all(np.isfinite(lo))
    xl = Xc.astype(LD)
    k1 = _cov(kern, ((xl - X[0].astype(LD)) ** 2).sum(1))
    k2 = _cov(kern, ((xl - X[1].astype(LD)) ** 2).sum(1))
    k12 = k1[1]
    # full[0] = A1 + A2 k12, full[1] = A1 k12 + A2
    A1 = (LD(full[0]) - k12 * LD(full[1])) / (1 - k12 * k12)
    A2 = (LD(full[1]) - k12 * LD(full[0])) / (1 - k12 * k12)
    mu = A1 * k1 + A2 * k2
    assert np.max(np.abs(mu - full.astype(LD))) <= 1e-11 * float(abs(A1) + abs(A2))      # the harness itself
    return (-(up + lo) / 2).astype(LD), mu, float(abs(A1) + abs(A2)), step


def _grid_candidates(D):
    """asymmetric integer candidates: around the first row with the lower digits at -128 and 127, and the box's corners"""
    A = _row_digits(D)
    rs = np.random.RandomState(3)
    ends = np.array([-128, 127])
    out = []
    for top in (-3, -1, 0, 1, 2):                       # the top digit near the row's: r up to a few length scales
        for rep in range(6):
            d1, d2 = ends[rs.randint(0, 2, D)], ends[rs.randint(0, 2, D)]
            if rep == 0:
                d1[:], d2[:] = -128, -128
            elif rep == 1:
                d1[:], d2[:] = 127, 127
            a0 = np.rint(A / 65536.0).astype(np.int64) + top * (1 + (np.arange(D) % 2))
            out.append(np.clip(a0, -128, 127) * 65536 + d1 * 256 + d2)
    for v in (-128, 127):                               # every digit of every dimension at one end; mixed corners
        out.append(np.full(D, v * 65536 + v * 256 + v))
        out.append(np.where(np.arange(D) % 2 == 0, 1, -1) * (127 * 65536 + 127 * 256 + 127))
    out.append(np.full(D, GRID))
    out.append(np.full(D, -GRID))
    out.append(A + np.arange(D) + 1)                    # next to the row: r2 of a few grid steps
    out.append(A.copy())
    B = np.array(out, dtype=np.int64)
    assert np.all(np.abs(B) <= 128 * 65793)
    return np.clip(B, -AMAX, AMAX)


def _check_exact(ctx, kern, D):
    mu_i, mu, asum, h = _pair(ctx, kern, D, _grid_candidates(D))
    err = float(np.max(np.abs(mu_i - mu))) / asum
    allowed = E1 + C2[kern] * 2.0 ** 20 * h * h
    print("%s D=%d on the grid: max |mu~ - mu| / (|A1| + |A2|) = %.3e (allowed %.3e)" % (kern, D, err, allowed))
    assert err <= allowed, (kern, D, err)


def _check_bound(ctx, kern, D):
    rs = np.random.RandomState(4)
    H = 0.25
    off = np.concatenate([rs.uniform(-2 * H, 2 * H, (160, D)), rs.uniform(-H, H, (80, D)) * 0.02 + 2.0 * H / GRID * _row_digits(D),
                          np.full((1, D), H), np.full((1, D), -H), np.full((1, D), 2 * H), np.full((1, D), -2 * H),
                          np.where(np.arange(D) % 2 == 0, 2 * H, -H)[None, :]])
    mu_i, mu, asum, h = _pair(ctx, kern, D, np.zeros_like(off), off_grid=off)
    err = float(np.max(np.abs(mu_i - mu))) / asum
    allowed = E1 + C2[kern] * 2.0 ** 20 * h * h + C1[kern] * np.sqrt(D) * h
    print("%s D=%d off the grid: max |mu~ - mu| / (|A1| + |A2|) = %.3e (allowed %.3e, grid term %.3e)" %
          (kern, D, err, allowed, C1[kern] * np.sqrt(D) * h))
    assert err <= allowed, (kern, D, err)


@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("D", (1, 3, 8, 16))
def test_exact_on_grid_emu(emu_ctx, D, kern):
    _check_exact(emu_ctx, kern, D)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("D", (1, 3, 8, 16))
def test_exact_on_grid_gpu(gpu_ctx, D, kern):
    _check_exact(gpu_ctx, kern, D)


@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("D", (1, 3, 8, 16))
def test_bound_emu(emu_ctx, D, kern):
    _check_bound(emu_ctx, kern, D)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("D", (1, 3, 8, 16))
def test_bound_gpu(gpu_ctx, D, kern):
    _check_bound(gpu_ctx, kern, D)


# ---- 2. edges of the tiling ------------------------------------------------------------------------------------------------------
def _check_edges(ctx, c, label):
    with TS._single(ctx, 2), _int(ctx, 1):
        up, lo = c.gp.screen_bounds("lcb", 0.0, 0.0, c.cand)
        assert c.cand.screen_form()[0] == FORM_INT8 and c.cand.bounds_kernel() == TD.DOT, label
        assert not np.isnan(up).any() and not np.isnan(lo).any(), label
        err, delta = np.abs(-(up + lo) / 2 - c.mu), (up - lo) / 2
        print("%s: max |mu~ - mu_sweep| in units of delta %.3e (allowed %.3f)" % (label, float((err / delta).max()), 1 / SAFETY))
        assert np.all(err <= delta / SAFETY), label
        TD._brackets(c, label)
        first = [c.gp.screen_bounds(kind, par, c.eta, c.cand) for kind, par in ACQS]
    with TS._single(ctx, 0):
        fp64 = [c.gp.screen_bounds(kind, par, c.eta, c.cand) for kind, par in ACQS]
        assert c.cand.screen_form() == (FORM_FP64, 0.0)
    for (kind, _), (u1, l1), (u0, l0) in zip(ACQS, first, fp64):
        s1, s0 = TS._survivors(u1, l1), TS._survivors(u0, l0)
        assert np.all(s1[s0]), (label, kind, int((s0 & ~s1).sum()))


@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("shape", EDGES, ids=_sid)
def test_edges_emu(emu_ctx, shape, kern):
    _check_edges(emu_ctx, _case(emu_ctx, shape, kern), "%s %s" % (kern, _sid(shape)))


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("shape", EDGES, ids=_sid)
def test_edges_gpu(gpu_ctx, shape, kern):
    _check_edges(gpu_ctx, _case(gpu_ctx, shape, kern), "%s %s" % (kern, _sid(shape)))


def _check_d17(ctx):
    c = _case(ctx, dict(N=257, D=17, M=200), "matern52")
    with TS._single(ctx, 2), _int(ctx, 1):
        c.gp.screen_bounds("lcb", 0.0, 0.0, c.cand)
        assert c.cand.screen_form() == (FORM_FP64, 0.0) and c.cand.bounds_kernel() == TD.DOT
    with TS._single(ctx, 1), _int(ctx, 1):
        c.refit()
        c.gp.acq("ei", 0.0, c.eta, c.cand, want_values=False)
        assert c.cand.screen_first()[0] in (1, 2) and c.cand.screen_form()[0] == FORM_FP64


def test_d17_emu(emu_ctx):
    _check_d17(emu_ctx)


@pytest.mark.gpu
def test_d17_gpu(gpu_ctx):
    _check_d17(gpu_ctx)


# ---- 3. same answer, bit for bit ---------------------------------------------------------------------------------------------------
def _argmax_only(ctx, c, kind, par, eta, key, refit=True):
    with TS._single(ctx, 1), _int(ctx, key):
        if refit:
            c.refit()
        out = c.gp.acq(kind, par, eta, c.cand, want_values=False)[1:]
        return out, c.cand.last_screen(), c.cand.screen_first(), c.cand.screen_form()[0]


def _same(a, b):
    return (_bits([a[0]], [b[0]]) or (np.isnan(a[0]) and np.isnan(b[0]))) and a[1:] == b[1:]


def _check_answers(ctx, c, label, must_survive=()):
    cap = max(1, c.M * 25 // 100)
    for kind, par in ACQS:
        with TD._tuned(ctx, "acq_screen", 0, None):
            off = c.gp.acq(kind, par, c.eta, c.cand, want_values=False)[1:]
        on0, scr0, first0, form0 = _argmax_only(ctx, c, kind, par, c.eta, 0)
        on1, scr1, first1, form1 = _argmax_only(ctx, c, kind, par, c.eta, 1)
        print("%s %s: key 0 stage %d kept %d; key 1 stage %d kept %d; solved %d / %d" %
              (label, kind, first0[0], first0[1], first1[0], first1[1], scr1[1], scr0[1]))
        assert form0 == FORM_FP64 and form1 == FORM_INT8 and first1[0] in (1, 2), (kind, form0, form1, first1)
        assert _same(on0, off) and _same(on1, off), (kind, on0, on1, off)
        if first1[0] == 1:
            assert scr1[1] == first1[1] and 1 <= first1[1] <= min(128, cap), (kind, scr1, first1)
        else:
            assert not (1 <= first1[1] <= min(128, cap)), (kind, first1)
        with TS._single(ctx, 2), _int(ctx, 1):
            u1, l1 = c.gp.screen_bounds(kind, par, c.eta, c.cand)
        with TS._single(ctx, 0):
            u0, l0 = c.gp.screen_bounds(kind, par, c.eta, c.cand)
        s1, s0 = TS._survivors(u1, l1), TS._survivors(u0, l0)
        assert np.all(s1[s0]), (label, kind)
        for i in must_survive:
            assert s1[i], (label, kind, i, u1[i])


def _check_many(ctx):
    _check_answers(ctx, _case(ctx, MANY, "matern52"), "N256 M4099")


def _check_strays(ctx, kern):
    c = TD._Case(ctx, 130, 5, 200, kern)
    with TS._single(ctx, 2), _int(ctx, 1):
        c.gp.screen_bounds("lcb", 0.0, 0.0, c.cand)
        h = c.cand.screen_form()[1]
    ell = np.exp(0.5 * c.theta[1])
    Xs = c.X / ell
    ctr = 0.5 * (Xs.max(0) + Xs.min(0))
    c.Xc[3] = 1e20
    c.Xc[5, 2], c.Xc[9, 0], c.Xc[11, 4] = np.nan, np.inf, -np.inf
    c.Xc[13, 1] = (ctr[1] + (AMAX + 2) * h) * ell           # just outside the digits' range
    c.cand.close()
    c.cand = _lib.Candidates(ctx, c.Xc)
    _check_answers(ctx, c, "%s strays" % kern, must_survive=(3, 5, 9, 11, 13))
    c.close()


def _check_pause(ctx):
    c = _case(ctx, MANY, "matern52")
    eta = c.eta - 1.0
    with TD._tuned(ctx, "acq_screen", 0, None):
        off = c.gp.acq("ei", 0.0, eta, c.cand, want_values=False)[1:]
    seq = {}
    for key in (0, 1):
        seq[key] = []
        for call in range(5):
            on, scr, (stage, _), form = _argmax_only(ctx, c, "ei", 0.0, eta, key, refit=(call == 0))
            assert _same(on, off) and scr[2] == _lib.SCREEN_PROBE_USED, (key, call, on, off, scr)
            assert form == (key if stage else FORM_FP64), (key, call, stage, form)
            seq[key].append(stage)
    assert seq[0] == seq[1] == [2, 0, 2, 0, 0], seq


def test_answers_emu(emu_ctx):
    _check_many(emu_ctx)


@pytest.mark.gpu
def test_answers_gpu(gpu_ctx):
    _check_many(gpu_ctx)


@pytest.mark.parametrize("kern", KERNELS)
def test_strays_emu(emu_ctx, kern):
    _check_strays(emu_ctx, kern)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNELS)
def test_strays_gpu(gpu_ctx, kern):
    _check_strays(gpu_ctx, kern)


def test_pause_emu(emu_ctx):
    _check_pause(emu_ctx)


@pytest.mark.gpu
def test_pause_gpu(gpu_ctx):
    _check_pause(gpu_ctx)


# ---- 4. the rule ---------------------------------------------------------------------------------------------------------------------
def _check_rule(ctx):
    # a length scale of e^-12: the scaled rows span 1.6e5, h = 0.02, the grid's term alone is several prior standard deviations
    s = dict(N=130, D=3, M=257)
    th = np.concatenate([[0.0], np.full(s["D"], -24.0), [np.log(1e-3)]])
    c = TD._Case(ctx, s["N"], s["D"], s["M"], "matern52", theta=th)
    for key, want in ((-1, FORM_FP64), (1, FORM_INT8), (0, FORM_FP64)):
        with TS._single(ctx, -1), _int(ctx, key):
            c.refit()
            c.gp.acq("ei", 0.0, c.eta, c.cand, want_values=False)
            stage, form = c.cand.screen_first()[0], c.cand.screen_form()[0]
            print("wide extent, key %d: stage %d, form %d" % (key, stage, form))
            assert stage in (1, 2) and form == want, (key, stage, form)
    c.close()
    # the benchmark's kind of fit: the rule takes the integer form from four k-steps of the fp64 form on (8 < D <= 16)
    for shape, want in ((MANY, FORM_INT8), (dict(N=129, D=8, M=65), FORM_FP64)):
        c = _case(ctx, shape, "matern52")
        with TS._single(ctx, -1), _int(ctx, -1):
            c.refit()
            c.gp.acq("ei", 0.0, c.eta, c.cand, want_values=False)
            assert c.cand.screen_first()[0] in (1, 2) and c.cand.screen_form()[0] == want, (shape, c.cand.screen_form())
    # one row has no extent: the rule keeps the fp64-MFMA form, key 1 takes the fall-back grid
    c = _case(ctx, dict(N=1, D=1, M=63), "matern52")
    for key, want in ((-1, FORM_FP64), (1, FORM_INT8)):
        with TS._single(ctx, 2), _int(ctx, key):
            c.gp.screen_bounds("lcb", 0.0, 0.0, c.cand)
            assert c.cand.screen_form()[0] == want, (key, c.cand.screen_form())


def test_rule_emu(emu_ctx):
    _check_rule(emu_ctx)


@pytest.mark.gpu
def test_rule_gpu(gpu_ctx):
    _check_rule(gpu_ctx)
