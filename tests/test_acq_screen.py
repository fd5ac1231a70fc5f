"""The acquisition screen of argmax-only sweeps (robo_amd/csrc/screen.hip: robo_acq_eval_cand and its sharded / multi-device
forms with out_acq == NULL, robo_cand_last_screen, robo_acq_screen_bounds).

CPU: through the interpreter (tests/hipemu) with `acq_screen_min` lowered so that the small shapes reach the screen.
-m gpu: the same checks at the same shapes on the MI355X, plus N = 256, D = 16, M = 65 539 at the default threshold.

Inputs: bench.py's synthetic() recipe with default_theta (Fabolas: one more uniform fidelity column on both sides, basis
weights a = 0.8, b = 1.3), and for the bounds the prior-edge thetas of tests/cov_checks.py (ln m in {-10, -4} x noise in
{e^-13, 1e-3}; for the Fabolas kind the same with the two basis weights).  The probe: N = 256, D = 16, M = 4099, eta - 1.
Seeds: candidates are RandomState(1 + rank) with rank 0, except rbf at N = 200, D = 3: there the fitted
surface leaves no candidate below the incumbent at rank 0 (max EI 9.4e-8; every upper bound reaches the best lower bound
in exact arithmetic as well, the regime DESIGN.md describes) and rank 2 is used.

The margins (screen.hip SCREEN_DELTA_REL, SCREEN_RHO) and what they were set from:
  delta = 1e-11 x scale,  scale = |y_mean| + y_std (|mean_c| + sqrt(k_cc) sum_j |alpha_j| sqrt(k_jj)).
      Measured max |mu~ - mu_sweep| over the shapes, kinds and thetas above (mu~ = k_* . alpha of the screen, read back
      through the LCB bounds at kappa = 0, which carry no rho; mu_sweep = the block-row substitution's mean), in units of
      delta:
          interpreter   1.2e-5         MI355X   1.1e-5        (|mu~ - mu| itself: at most 1.1e-11 here, 2.2e-11 at N = 4096)
      i.e. 1.2e-16 of the scale: delta is 8e4 x the largest difference seen (the floor the issue sets is 1000 x).
      test_bounds_* print every figure and assert the ratio <= 1e-3.
  rho = 1e-5, relative, on the prior variance and on the value of EI, PI and LogEI (LogEI: of |value| + 1; LCB is a plain
      sum and takes none).  Measured: how far a value FALLS when its arguments move one step in the direction that must
      raise it (mean down by 4 ulp, variance up by 4 ulp), relative to the value, over z in [-37, 8] x sigma in
      {1e-3, 0.1, 1}:
          interpreter   EI 3.4e-10   LogEI 2.2e-13   PI 0         LCB 0
          MI355X        EI 3.4e-10   LogEI 2.2e-13   PI 2.1e-16   LCB 0
      EI's figure is eps z^4 at z = -37: the argument of erfc carries eps, Phi(z) answers with 2 (z^2 / 2) eps, and the
      cancellation of z Phi(z) + phi(z) multiplies by z^2 once more.  rho is 3e4 x the largest; test_value_spread_* assert
      1000 x measured <= rho.
  Guard: max L_ii / min L_ii <= 1e4.  The thetas above reach 32; an rbf factor at the noise floor (noise 1e-13 + jitter,
      test_guards_*) reaches 4.6e4: there |mu~ - mu_sweep| is 1.0e-5 (interpreter) / 8.7e-6 (MI355X), still 3e-5 of a
      delta that |alpha|_1 has driven to 0.3 -- sound, but such a delta prunes nothing, so the screen is not tried.
"""
import os
import sys

import numpy as np
import pytest

from robo_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cov_checks as CC  # noqa: E402
from bench import synthetic  # noqa: E402

SCREEN_RHO = 1e-5
SHAPES = (dict(N=80, D=3, M=400), dict(N=200, D=3, M=1000), dict(N=300, D=8, M=1000))
LARGE = dict(N=256, D=16, M=65539)          # tests/test_mes.py LARGE
KERNELS = ("matern52", "rbf", "fabolas")
ACQS = (("ei", 0.0), ("log_ei", 0.0), ("pi", 0.0), ("lcb", 1.0))
SCREEN_MIN = 100


def _emu_env():
    sys.path.insert(0, os.path.join(HERE, "hipemu"))
    import build_emu
    return build_emu.build(), build_emu.build_fake_rccl()


@pytest.fixture(scope="module")
def emu_ctx():
    lib_path, rccl_path = _emu_env()
    old = {k: os.environ.get(k) for k in ("HIPEMU_DEVICES", "ROBO_RCCL_LIB")}
    os.environ["HIPEMU_DEVICES"] = "2"
    os.environ["ROBO_RCCL_LIB"] = rccl_path
    _lib.use_library(lib_path)
    ctx = _lib.Context(0)
    assert "hipemu" in ctx.name
    ctx.set_tuning("acq_screen_min", SCREEN_MIN)
    yield ctx
    _CACHE.clear()
    ctx.close()
    _lib.use_library(None)
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


@pytest.fixture(scope="module")
def gpu_ctx():
    _lib.use_library(None)
    if _lib.device_count() < 1:
        pytest.skip("no HIP device")
    ctx = _lib.Context(0)
    ctx.set_tuning("acq_screen_min", SCREEN_MIN)
    yield ctx
    _CACHE.clear()
    ctx.close()


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _inputs(N, D, M, kern):
    rank = 2 if (kern, N, D) == ("rbf", 200, 3) else 0          # see the module docstring
    X, y, theta, Xc = synthetic(N, D, M, rank)
    if kern == "fabolas":
        X = np.hstack([X, np.random.RandomState(5).rand(N, 1)])
        Xc = np.hstack([Xc, np.random.RandomState(6).rand(M, 1)])
        theta = np.concatenate([theta[:-1], [np.log(0.8), np.log(1.3)], theta[-1:]])
    return X, y, theta, Xc


_CACHE = {}


class _Case(object):
    """a fitted GP, its resident candidates and, per acquisition, the unscreened sweep's values: computed once per module"""

    def __init__(self, ctx, N, D, M, kern, theta=None):
        self.ctx, self.M = ctx, M
        self.X, self.y, self.theta, self.Xc = _inputs(N, D, M, kern)
        if theta is not None:
            self.theta = theta
        self.mean_c, self.eta = float(np.mean(self.y)), float(self.y.min())
        self.gp = _lib.DeviceGP(ctx, kern, N, self.X.shape[1])
        self.gp.set_data(self.X, self.y)
        self.refit()
        self.cand = _lib.Candidates(ctx, self.Xc)
        self._values = {}

    def refit(self):
        self.gp.fit(self.theta, self.mean_c)

    def values(self, kind, par):
        if (kind, par) not in self._values:
            self._values[(kind, par)] = self.gp.acq(kind, par, self.eta, self.cand, want_values=True)
        return self._values[(kind, par)]


def _case(ctx, shape, kern):
    key = (id(ctx), shape["N"], shape["D"], shape["M"], kern)
    if key not in _CACHE:
        _CACHE[key] = _Case(ctx, shape["N"], shape["D"], shape["M"], kern)
    return _CACHE[key]


def _np_argmax(v):
    return int(np.flatnonzero(np.isnan(v))[0]) if np.isnan(v).any() else int(np.argmax(v))


def _unscreened(ctx, fn):
    ctx.set_tuning("acq_screen", 0)
    try:
        return fn()
    finally:
        ctx.set_tuning("acq_screen", None)


# ---- 1. same answer, bit for bit ---------------------------------------------------------------------------------------------
def _check_same_answer(ctx, shape, kern, acqs=ACQS):
    c = _case(ctx, shape, kern)
    for kind, par in acqs:
        vals, mx, am, fl = c.values(kind, par)
        off = _unscreened(ctx, lambda: c.gp.acq(kind, par, c.eta, c.cand, want_values=False)[1:])
        on = c.gp.acq(kind, par, c.eta, c.cand, want_values=False)[1:]
        n, kept, outcome = c.cand.last_screen()
        print("%s N=%d D=%d M=%d %s: kept %d of %d, outcome %d" % (kern, shape["N"], shape["D"], shape["M"], kind, kept, n,
                                                                   outcome))
        assert _bits([on[0]], [off[0]]) and on[1:] == off[1:], (kind, on, off)
        assert _bits([on[0]], [mx]) and on[1:] == (am, fl)
        assert on[1] == _np_argmax(vals) and _bits([on[0]], vals[on[1]:on[1] + 1])
        assert outcome == _lib.SCREEN_SCREENED and n == c.M and 1 <= kept <= c.M // 4, (kind, n, kept, outcome)


@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d" % s["N"])
def test_same_answer_emu(emu_ctx, shape, kern):
    _check_same_answer(emu_ctx, shape, kern)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("shape", SHAPES + (LARGE,), ids=lambda s: "N%d" % s["N"])
def test_same_answer_gpu(gpu_ctx, shape, kern):
    if shape is LARGE:
        gpu_ctx.set_tuning("acq_screen_min", None)       # the default threshold: above winv_max
    try:
        _check_same_answer(gpu_ctx, shape, kern)
    finally:
        gpu_ctx.set_tuning("acq_screen_min", SCREEN_MIN)


def _check_sharded_and_multi(ctx, devices):
    shape = SHAPES[1]
    c = _case(ctx, shape, "matern52")
    vals, mx, am, fl = c.values("log_ei", 0.0)
    comm = _lib.Comm(ctx, 0, 1, _lib.Comm.create_id())
    try:
        off = _unscreened(ctx, lambda: comm.acq_sharded(c.gp, "log_ei", 0.0, c.eta, c.cand, 1000))
        c.refit()
        on = comm.acq_sharded(c.gp, "log_ei", 0.0, c.eta, c.cand, 1000)
        n, kept, outcome = c.cand.last_screen()
        assert on[0] is None and _bits([on[1]], [off[1]]) and on[2:] == off[2:]
        assert _bits([on[1]], [mx]) and on[2:] == (am + 1000, 0, fl)
        assert outcome == _lib.SCREEN_SCREENED and n == c.M and kept <= c.M // 4
    finally:
        comm.close()
    multi = _lib.multi_for(devices)
    for mctx in multi.ctxs:
        mctx.set_tuning("acq_screen_min", SCREEN_MIN)
    gps = [_lib.DeviceGP(mc, "matern52", shape["N"], shape["D"]) for mc in multi.ctxs]
    multi.set_data(gps, c.X, c.y)
    multi.fit(gps, c.theta, c.mean_c)
    shards = _lib.CandidateShards.split(multi.ctxs, c.Xc)
    try:
        vals, mx, am, fl = c.values("ei", 0.0)
        for mctx in multi.ctxs:
            mctx.set_tuning("acq_screen", 0)
        off = multi.acq(gps, "ei", 0.0, c.eta, shards, want_values=False)
        for mctx in multi.ctxs:
            mctx.set_tuning("acq_screen", None)
        on = multi.acq(gps, "ei", 0.0, c.eta, shards, want_values=False)
        assert _bits([on[1]], [off[1]]) and on[2:] == off[2:]
        assert _bits([on[1]], [mx]) and on[2] == am and on[4] == fl
        for sh in shards.shards:
            n, kept, outcome = sh.last_screen()
            assert outcome == _lib.SCREEN_SCREENED and n == sh.m and kept <= sh.m // 4
    finally:
        for mctx in multi.ctxs:
            mctx.set_tuning("acq_screen", None)
            mctx.set_tuning("acq_screen_min", None)
        shards.close()
        for g in gps:
            g.close()


def test_sharded_and_multi_emu(emu_ctx):
    _check_sharded_and_multi(emu_ctx, [0, 1])


@pytest.mark.gpu
def test_sharded_and_multi_gpu(gpu_ctx):
    _check_sharded_and_multi(gpu_ctx, [0, 0])


# ---- 2. bounds are bounds ------------------------------------------------------------------------------------------------------
def _edge_thetas(D, kern):
    """tests/cov_checks.py's prior-edge thetas; the Fabolas layout carries its two basis weights before the noise"""
    extra = [np.log(0.8), np.log(1.3)] if kern == "fabolas" else []
    return [np.concatenate([[np.log(1.3)], np.full(D, lnm), extra, [np.log(noise)]])
            for lnm in CC.FEED_LNM for noise in CC.FEED_NOISE]


def _check_one_bounds(ctx, c, label):
    # the mean of the screen against the sweep's, in units of the screen's own delta: LCB at kappa = 0 is -mean
    mu, _ = _unscreened(ctx, lambda: c.gp.predict(c.cand))
    up, lo = c.gp.screen_bounds("lcb", 0.0, 0.0, c.cand)
    ratio = float((np.abs(-(up + lo) / 2 - mu) / ((up - lo) / 2)).max())
    print("%s: max |mu~ - mu_sweep| = %.3e, in units of delta %.3e" % (label, np.abs(-(up + lo) / 2 - mu).max(), ratio))
    assert ratio <= 1e-3, (label, ratio)          # delta is at least 1000 x what is seen
    for kind, par in ACQS:
        vals = c.values(kind, par)[0]
        up, lo = c.gp.screen_bounds(kind, par, c.eta, c.cand)
        assert not np.isnan(up).any() and not np.isnan(lo).any() and not np.isnan(vals).any(), (label, kind)
        assert np.all(lo <= vals) and np.all(vals <= up), (label, kind, int((lo > vals).sum()), int((vals > up).sum()))
    return ratio


def _check_bounds(ctx, shape, kern):
    c = _case(ctx, shape, kern)
    worst = _check_one_bounds(ctx, c, "%s N=%d default theta" % (kern, shape["N"]))
    for th in _edge_thetas(shape["D"], kern):
        e = _Case(ctx, shape["N"], shape["D"], shape["M"], kern, theta=th)
        worst = max(worst, _check_one_bounds(ctx, e, "%s N=%d ln m=%g noise=%.3g" % (kern, shape["N"], th[1], np.exp(th[-1]))))
        e.cand.close()
        e.gp.close()
    # NaN inputs give NaN bounds, for that candidate alone.  (The Fabolas product kernel turns a NaN in an INPUT column
    # into the factor 0 -- matern52_1d's `e > 0 ? ... : 0` -- in the sweep and in the screen alike: a NaN value arises
    # from its fidelity column only, so the NaN goes into the last column; the first column is the bracket's business.)
    Xn = c.Xc.copy()
    Xn[7, -1] = np.nan
    Xn[9, 0] = np.nan
    cn = _lib.Candidates(ctx, Xn)
    for kind, par in ACQS:
        vals = c.gp.acq(kind, par, c.eta, cn, want_values=True)[0]
        up, lo = c.gp.screen_bounds(kind, par, c.eta, cn)
        nan = np.isnan(vals)
        assert nan[7] and nan.sum() == (1 if kern == "fabolas" else 2), kind
        assert np.array_equal(np.isnan(up), nan) and np.array_equal(np.isnan(lo), nan), kind
        assert np.all(lo[~nan] <= vals[~nan]) and np.all(vals[~nan] <= up[~nan]), kind
    cn.close()
    with pytest.raises(Exception):
        c.gp.screen_bounds("lcb", -1.0, 0.0, c.cand)
    print("worst |mu~ - mu| / delta: %.3e" % worst)


@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d" % s["N"])
def test_bounds_emu(emu_ctx, shape, kern):
    _check_bounds(emu_ctx, shape, kern)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("shape", SHAPES + (LARGE,), ids=lambda s: "N%d" % s["N"])
def test_bounds_gpu(gpu_ctx, shape, kern):
    _check_bounds(gpu_ctx, shape, kern)


def _check_value_spread(ctx):
    """how far acq_* falls when its arguments move a step in the direction that must raise it: rho covers 1000 x that"""
    eta = 0.3
    z = np.linspace(-37.0, 8.0, 4501)
    worst = {}
    for kind, par in ACQS:
        w = 0.0
        for s in (1e-3, 0.1, 1.0):
            m = eta - par - z * s if kind != "lcb" else -z
            v = np.full_like(m, s * s)
            m1 = m - 4 * np.spacing(np.abs(m))
            v1 = v * (1 + 4 * np.finfo(float).eps)
            if kind == "pi":                       # PI rises with sigma only where its numerator is negative
                v1 = np.where(eta - par - m1 < 0, v1, v)
            a0 = _lib.acq_from_moments(ctx, kind, par, eta, m, v)[0]
            a1 = _lib.acq_from_moments(ctx, kind, par, eta, m1, v1)[0]
            scale = np.abs(a0) + (1.0 if kind == "log_ei" else 0.0)
            with np.errstate(invalid="ignore", divide="ignore"):
                fall = np.where(scale > 0, (a0 - a1) / scale, 0.0)
            w = max(w, float(np.nanmax(fall)))
        worst[kind] = w
    print("value spread: " + "  ".join("%s %.2e" % kv for kv in sorted(worst.items())))
    assert 1000 * max(worst.values()) <= SCREEN_RHO, worst


def test_value_spread_emu(emu_ctx):
    _check_value_spread(emu_ctx)


@pytest.mark.gpu
def test_value_spread_gpu(gpu_ctx):
    _check_value_spread(gpu_ctx)


# ---- 3. / 4. / 5. ties, NaN, nothing to prune -----------------------------------------------------------------------------------
def _on_off(ctx, c, cand, kind, par, eta):
    off = _unscreened(ctx, lambda: c.gp.acq(kind, par, eta, cand, want_values=False)[1:])
    c.refit()                                      # every comparison starts without a back-off
    on = c.gp.acq(kind, par, eta, cand, want_values=False)[1:]
    assert (np.isnan(on[0]) and np.isnan(off[0])) or _bits([on[0]], [off[0]])
    assert on[1:] == off[1:], (on, off)
    return on, cand.last_screen()


def _check_ties_nan_nothing(ctx):
    shape = SHAPES[1]
    c = _case(ctx, shape, "matern52")
    M = c.M
    am = c.values("ei", 0.0)[2]
    # the winner duplicated at a lower and a higher index: the lowest index
    lo_i, hi_i = (3, M - 5) if am not in (3, M - 5) else (4, M - 6)
    assert lo_i < am < hi_i
    Xt = c.Xc.copy()
    Xt[lo_i] = Xt[am]
    Xt[hi_i] = Xt[am]
    ct = _lib.Candidates(ctx, Xt)
    on, (n, kept, outcome) = _on_off(ctx, c, ct, "ei", 0.0, c.eta)
    assert on[1] == lo_i and outcome == _lib.SCREEN_SCREENED and kept >= 3
    ct.close()
    # every EI exactly 0 (eta far below every mean): index 0, and nothing could be pruned
    on, (n, kept, outcome) = _on_off(ctx, c, c.cand, "ei", 0.0, c.eta - 1e3)
    assert on[0] == 0.0 and on[1] == 0 and outcome == _lib.SCREEN_FELL_BACK and (n, kept) == (M, M)
    # a NaN coordinate: that index, NaN, the flag
    Xn = c.Xc.copy()
    Xn[M // 2, 1] = np.nan
    cn = _lib.Candidates(ctx, Xn)
    on, (n, kept, outcome) = _on_off(ctx, c, cn, "ei", 0.0, c.eta)
    assert np.isnan(on[0]) and on[1] == M // 2 and on[2] & _lib.FLAG_NAN and outcome == _lib.SCREEN_SCREENED
    cn.close()
    # nothing to prune: identical candidates; LCB with a huge kappa
    cs = _lib.Candidates(ctx, np.tile(c.Xc[:1], (M, 1)))
    on, (n, kept, outcome) = _on_off(ctx, c, cs, "lcb", 1.0, 0.0)
    assert on[1] == 0 and outcome == _lib.SCREEN_FELL_BACK and kept == M
    on, (n, kept, outcome) = _on_off(ctx, c, c.cand, "lcb", 1e6, 0.0)
    assert outcome == _lib.SCREEN_FELL_BACK and kept > M // 4
    # the back-off: the next call on the same factor does not screen, the one after it does; a refit screens at once
    ref = c.gp.acq("lcb", 1e6, 0.0, c.cand, want_values=False)[1:]
    assert ref == on and c.cand.last_screen() == (0, 0, _lib.SCREEN_NOT_ELIGIBLE)
    c.gp.acq("lcb", 1e6, 0.0, c.cand, want_values=False)
    assert c.cand.last_screen()[2] == _lib.SCREEN_FELL_BACK
    for _ in range(2):                             # ... and now two calls pass unscreened
        c.gp.acq("lcb", 1e6, 0.0, c.cand, want_values=False)
        assert c.cand.last_screen() == (0, 0, _lib.SCREEN_NOT_ELIGIBLE)
    c.refit()
    c.gp.acq("lcb", 1e6, 0.0, c.cand, want_values=False)
    assert c.cand.last_screen()[0] == M
    cs.close()
    c.refit()


def test_ties_nan_nothing_to_prune_emu(emu_ctx):
    _check_ties_nan_nothing(emu_ctx)


@pytest.mark.gpu
def test_ties_nan_nothing_to_prune_gpu(gpu_ctx):
    _check_ties_nan_nothing(gpu_ctx)


# ---- the probe: eta below every mean by about one prior sigma --------------------------------------------------------------------
PROBE = dict(N=256, D=16, M=4099)


def _check_probe(ctx):
    """max L is the value at the variance floor (~0) and prunes nothing; the exact values of the 128 candidates with the
    largest upper bounds do (the issue's restatement: 172 of 4099 kept for EI at this shape with eta - 1)"""
    c = _Case(ctx, PROBE["N"], PROBE["D"], PROBE["M"], "matern52")
    eta = c.eta - 1.0
    for kind in ("ei", "log_ei", "pi"):
        vals, mx, am, fl = c.gp.acq(kind, 0.0, eta, c.cand, want_values=True)
        on, (n, kept, outcome) = _on_off(ctx, c, c.cand, kind, 0.0, eta)
        print("probe %s: kept %d of %d, outcome %d" % (kind, kept, n, outcome))
        assert _bits([on[0]], [mx]) and on[1:] == (am, fl) and am == _np_argmax(vals)
        assert outcome == _lib.SCREEN_PROBE_USED and n == c.M and 1 <= kept <= c.M // 4, (kind, n, kept, outcome)
        up, lo = c.gp.screen_bounds(kind, 0.0, eta, c.cand)
        assert int((up >= lo.max()).sum()) > c.M // 4          # without the probe the call would have fallen back
    c.cand.close()
    c.gp.close()


def test_probe_emu(emu_ctx):
    _check_probe(emu_ctx)


@pytest.mark.gpu
def test_probe_gpu(gpu_ctx):
    _check_probe(gpu_ctx)


# ---- 6. guards -----------------------------------------------------------------------------------------------------------------
def _same_result(a, b):
    for k, v in vars(a).items():
        w = getattr(b, k)
        if isinstance(v, np.ndarray):
            assert v.dtype == w.dtype and v.shape == w.shape and v.tobytes() == w.tobytes(), k
        else:
            assert v == w or (v != v and w != w), k


def _check_guards(ctx):
    shape = SHAPES[0]
    c = _case(ctx, shape, "matern52")
    c.refit()
    not_eligible = (0, 0, _lib.SCREEN_NOT_ELIGIBLE)
    c.gp.acq("lcb", -1.0, 0.0, c.cand, want_values=False)                 # kappa < 0: no monotone bound
    assert c.cand.last_screen() == not_eligible
    c.gp.acq("ei", 0.0, c.eta, c.cand, want_values=True)                  # the caller takes the values
    assert c.cand.last_screen() == not_eligible
    c.gp.acq("ei", 0.0, float("inf"), c.cand, want_values=False)
    assert c.cand.last_screen() == not_eligible
    ctx.set_tuning("acq_screen_min", c.M)                                  # batches ABOVE the key
    c.gp.acq("ei", 0.0, c.eta, c.cand, want_values=False)
    assert c.cand.last_screen() == not_eligible
    ctx.set_tuning("acq_screen_min", c.M - 1)
    c.gp.acq("ei", 0.0, c.eta, c.cand, want_values=False)
    assert c.cand.last_screen()[2] == _lib.SCREEN_SCREENED
    ctx.set_tuning("acq_screen_min", SCREEN_MIN)
    # a factor at the noise floor, beyond the conditioning guard
    floor = _Case(ctx, shape["N"], shape["D"], shape["M"], "rbf", theta=np.concatenate([c.theta[:-1], [np.log(1e-13)]]))
    cond = floor.gp.factor_cond()
    assert cond[2] > 1e4 * cond[1]
    mu, _ = _unscreened(ctx, lambda: floor.gp.predict(floor.cand))
    up, lo = floor.gp.screen_bounds("lcb", 0.0, 0.0, floor.cand)
    print("beyond the guard (max L_ii / min L_ii = %.3g): max |mu~ - mu_sweep| = %.3e, in units of delta %.3e" % (
        cond[2] / cond[1], np.abs(-(up + lo) / 2 - mu).max(), (np.abs(-(up + lo) / 2 - mu) / ((up - lo) / 2)).max()))
    off = _unscreened(ctx, lambda: floor.gp.acq("ei", 0.0, floor.eta, floor.cand, want_values=False))
    on = floor.gp.acq("ei", 0.0, floor.eta, floor.cand, want_values=False)
    assert floor.cand.last_screen() == not_eligible, cond
    assert on[2:] == off[2:] and _bits([on[1]], [off[1]])
    floor.cand.close()
    floor.gp.close()
    # the ensemble drivers keep their own sweep: same results with the key on and off
    u = np.random.RandomState(3).rand(8)
    rep = _lib.Candidates(ctx, np.random.RandomState(4).rand(10, shape["D"]))
    drivers = (lambda: c.gp.refine("ei", 0.0, c.eta, c.cand, n_starts=8, n_steps=3),
               lambda: _lib.acq_batch([c.gp], "ei", 0.0, c.eta, c.cand, 3, marginal=False),
               lambda: c.gp.mes(c.eta, c.cand, u, want_values=False),
               lambda: c.gp.kg(c.cand, rep, 1e-3, want_values=False))
    for fn in drivers:
        _same_result(_unscreened(ctx, fn), fn())
    rep.close()
    c.refit()


def test_guards_emu(emu_ctx):
    _check_guards(emu_ctx)


@pytest.mark.gpu
def test_guards_gpu(gpu_ctx):
    _check_guards(gpu_ctx)


# ---- 7. / 8. stale state, events -------------------------------------------------------------------------------------------------
def _check_stale_state(ctx):
    c = _case(ctx, SHAPES[1], "matern52")
    c.refit()
    ref = _unscreened(ctx, lambda: c.gp.predict(c.cand))
    c.gp.acq("ei", 0.0, c.eta, c.cand, want_values=False)
    assert c.cand.last_screen()[2] == _lib.SCREEN_SCREENED
    mu, var = c.gp.predict(c.cand)
    assert _bits(mu, ref[0]) and _bits(var, ref[1])
    # ... and a full sweep after a screened call returns every value
    c.gp.acq("ei", 0.0, c.eta, c.cand, want_values=False)
    vals = c.gp.acq("ei", 0.0, c.eta, c.cand, want_values=True)[0]
    assert _bits(vals, c.values("ei", 0.0)[0])


def test_stale_state_emu(emu_ctx):
    _check_stale_state(emu_ctx)


@pytest.mark.gpu
def test_stale_state_gpu(gpu_ctx):
    _check_stale_state(gpu_ctx)


def _check_events(shape, phase_events):
    """bench.py reads slots 25 -> 26 after every timed step: a screened call records them like the sweep of the same batch"""
    ctx = _lib.Context(0)
    try:
        if phase_events:                              # batches of <= 16 384 candidates record them on request only
            ctx.set_phase_events(True)
            ctx.set_tuning("acq_screen_min", SCREEN_MIN)
        c = _Case(ctx, shape["N"], shape["D"], shape["M"], "matern52")
        c.gp.acq("ei", 0.0, c.eta, c.cand, want_values=False)
        assert c.cand.last_screen()[2] == _lib.SCREEN_SCREENED
        assert ctx.elapsed_ms(25, 26) >= 0.0
        assert c.cand.solve_kernel() == "trsm_step_small_kernel"
        c.cand.close()
        c.gp.close()
    finally:
        ctx.close()


def test_events_emu(emu_ctx):
    _check_events(SHAPES[0], True)
    # more than 16 384 candidates: the sweep records the pair without being asked, and so must the screened call, whose
    # survivors are a small batch
    os.environ["ROBO_ACQ_SCREEN_MIN"] = str(SCREEN_MIN)
    try:
        _check_events(dict(N=80, D=3, M=16500), False)
    finally:
        del os.environ["ROBO_ACQ_SCREEN_MIN"]


@pytest.mark.gpu
def test_events_gpu(gpu_ctx):
    _check_events(SHAPES[0], True)
    _check_events(LARGE, False)
