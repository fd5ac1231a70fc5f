"""The dot-form bounds kernel of the acquisition screen (robo_amd/csrc/screen.hip screen_bounds_dot_kernel, the tuning key
`acq_screen_dot`, the selection rule of launch_screen_bounds).

CPU: through the interpreter (tests/hipemu) with `acq_screen_min` lowered to 0 so that every shape reaches the screen.
-m gpu: the same checks at the same shapes on the MI355X, plus N = 256, D = 16, M = 65 539 at the default threshold.

Shapes: kinds matern52 and rbf; every N in {15, 130, 257} (a partial MFMA row tile, a partial 128-row stage, one row past a
stage edge), every D in {1, 3, 5, 16, 17} (K padded to a multiple of 4; the kernel's four k-loop lengths 1, 1, 2, 4 -- the tuned
case -- and 8: the limit is D = 32, so D = 17 runs the dot kernel too) and every M in {1, 65, 200, 1000} (a lone candidate, one past a
candidate tile of the workgroup, partial workgroups) occur in SHAPES; the cross product is not run.  Inputs: bench.py's
synthetic() recipe with default_theta.  Two more cases: candidate 3 equal to training row 7 (r2 = 0 after cancellation: the
clamp, no NaN) and the data shifted by +100 in every raw coordinate (the centring).  Every case runs with acq_screen_dot = 1,
and with 0 where a comparison is named.

What is asserted:
  bounds      U_c >= the unscreened sweep's value >= L_c for EI, LogEI, PI and LCB kappa = 1, every candidate;
  mu~         |mu~ - mu_sweep| <= 1e-4 of the delta the kernel applied (mu~ and delta read back through the LCB bounds at
              kappa = 0; the reference is the block-row sweep's mean, never the dot kernel);
  prior edge  tests/cov_checks.py's thetas (ln m in {-10, -4}): with acq_screen_dot = -1 the rule sends ln m = -10 to the
              direct kernel and the bounds are byte-identical to acq_screen_dot = 0; with 1 the bounds still bracket the
              sweep's values (the per-candidate delta term);
  identity    argmax-only calls return the unscreened (max, argmax, flags) bit for bit with acq_screen_dot at 1 and at 0,
              single-device, sharded on a one-rank communicator and multi-device on two devices; the survivors stay within
              the cap under the dot kernel wherever they do under the direct one;
  selection   the headline's and config 2's theta and extents take the dot kernel under the rule, Fabolas never does.

Measured (SCREEN_DOT_BOUND = 1e-12; `pytest -s` prints every figure):
  max |mu~ - mu_sweep| in units of delta, acq_screen_dot = 1, default theta, over SHAPES and the two extra cases:
      interpreter   1.5e-5      MI355X   1.3e-5        (|mu~ - mu| itself: at most 1.2e-11)
  the same under the rule at the prior edge's ln m = -4 (the largest r2 error the rule lets through, 5.3e-13 at D = 8):
      interpreter   2.6e-6      MI355X   2.9e-6
  i.e. delta is 6e4 x the largest difference seen (the floor the issue sets is 1e4 x).  Survivors: the direct kernel's count at
  every shape and acquisition, on the interpreter and on the MI355X (1 - 41 of 65 - 1000 where the screen prunes at all).
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

KERNELS = ("matern52", "rbf")
SHAPES = (dict(N=15, D=1, M=1), dict(N=15, D=3, M=65), dict(N=130, D=5, M=200), dict(N=257, D=16, M=1000),
          dict(N=130, D=17, M=65), dict(N=257, D=3, M=200), dict(N=130, D=1, M=1000), dict(N=15, D=16, M=200),
          dict(N=257, D=5, M=1), dict(N=257, D=17, M=200))
IDENTITY = dict(N=257, D=3, M=200)          # the sharded and the multi-device form
LARGE = dict(N=256, D=16, M=65539)          # tests/test_acq_screen.py LARGE
ACQS = (("ei", 0.0), ("log_ei", 0.0), ("pi", 0.0), ("lcb", 1.0))
DOT, DIRECT = "screen_bounds_dot_kernel", "screen_bounds_kernel"
MU_RATIO_MAX = 1e-4


def _sid(s):
    return "N%d-D%d-M%d" % (s["N"], s["D"], s["M"])


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
    ctx.set_tuning("acq_screen_min", 0)
    ctx.set_tuning("acq_screen_dot", 1)
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
    ctx.set_tuning("acq_screen_min", 0)
    ctx.set_tuning("acq_screen_dot", 1)
    yield ctx
    _CACHE.clear()
    ctx.close()


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


_CACHE = {}


class _Case(object):
    """a fitted GP, its resident candidates, the sweep's mean and, per acquisition, the unscreened sweep's values"""

    def __init__(self, ctx, N, D, M, kern, theta=None, shift=0.0, equal_row=False):
        self.ctx, self.M = ctx, M
        self.X, self.y, self.theta, self.Xc = synthetic(N, D, M, 0)
        if kern == "fabolas":
            self.X = np.hstack([self.X, np.random.RandomState(5).rand(N, 1)])
            self.Xc = np.hstack([self.Xc, np.random.RandomState(6).rand(M, 1)])
            self.theta = np.concatenate([self.theta[:-1], [np.log(0.8), np.log(1.3)], self.theta[-1:]])
        if equal_row:
            self.Xc[3] = self.X[7]
        self.X, self.Xc = self.X + shift, self.Xc + shift
        if theta is not None:
            self.theta = theta
        self.mean_c, self.eta = float(np.mean(self.y)), float(self.y.min())
        self.gp = _lib.DeviceGP(ctx, kern, N, self.X.shape[1])
        self.gp.set_data(self.X, self.y)
        self.refit()
        self.cand = _lib.Candidates(ctx, self.Xc)
        self.mu = self.gp.predict(self.cand)[0]
        self._values = {}

    def refit(self):
        self.gp.fit(self.theta, self.mean_c)

    def values(self, kind, par):
        if (kind, par) not in self._values:
            self._values[(kind, par)] = self.gp.acq(kind, par, self.eta, self.cand, want_values=True)
        return self._values[(kind, par)]

    def close(self):
        self.cand.close()
        self.gp.close()


def _case(ctx, shape, kern):
    key = (id(ctx), shape["N"], shape["D"], shape["M"], kern)
    if key not in _CACHE:
        _CACHE[key] = _Case(ctx, shape["N"], shape["D"], shape["M"], kern)
    return _CACHE[key]


class _tuned(object):
    """a tuning key at a value for the length of a block; back to what the fixture set afterwards"""

    def __init__(self, ctx, key, value, back):
        self.ctx, self.key, self.value, self.back = ctx, key, value, back

    def __enter__(self):
        self.ctx.set_tuning(self.key, self.value)

    def __exit__(self, *exc):
        self.ctx.set_tuning(self.key, self.back)


def _dot(ctx, value):
    return _tuned(ctx, "acq_screen_dot", value, 1)


# ---- bounds are bounds; mu~ against the sweep's mean -------------------------------------------------------------------------
def _mu_ratio(c, label):
    up, lo = c.gp.screen_bounds("lcb", 0.0, 0.0, c.cand)
    assert not np.isnan(up).any() and not np.isnan(lo).any(), label
    err, delta = np.abs(-(up + lo) / 2 - c.mu), (up - lo) / 2
    ratio = float((err / delta).max())
    print("%s [%s]: max |mu~ - mu_sweep| = %.3e, in units of delta %.3e" % (label, c.cand.bounds_kernel(), err.max(), ratio))
    return ratio


def _brackets(c, label):
    for kind, par in ACQS:
        vals = c.values(kind, par)[0]
        up, lo = c.gp.screen_bounds(kind, par, c.eta, c.cand)
        assert not np.isnan(up).any() and not np.isnan(lo).any() and not np.isnan(vals).any(), (label, kind)
        assert np.all(lo <= vals) and np.all(vals <= up), (label, kind, int((lo > vals).sum()), int((vals > up).sum()))


def _check_bounds(ctx, c, label, expect=DOT):
    ratio = _mu_ratio(c, label)
    assert c.cand.bounds_kernel() == expect, label
    assert ratio <= MU_RATIO_MAX, (label, ratio)
    _brackets(c, label)


@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_bounds_emu(emu_ctx, shape, kern):
    _check_bounds(emu_ctx, _case(emu_ctx, shape, kern), "%s %s" % (kern, _sid(shape)))


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_bounds_gpu(gpu_ctx, shape, kern):
    _check_bounds(gpu_ctx, _case(gpu_ctx, shape, kern), "%s %s" % (kern, _sid(shape)))


def _check_equal_row_and_shift(ctx, kern):
    s = dict(N=130, D=5, M=200)
    c = _Case(ctx, s["N"], s["D"], s["M"], kern, equal_row=True)
    _check_bounds(ctx, c, "%s candidate 3 = training row 7" % kern)
    c.close()
    c = _Case(ctx, s["N"], s["D"], s["M"], kern, shift=100.0)
    _check_bounds(ctx, c, "%s data + 100" % kern)
    with _dot(ctx, -1):                        # centred extents: the rule keeps the dot kernel for data far from the origin
        _check_bounds(ctx, c, "%s data + 100, the rule" % kern)
    c.close()


@pytest.mark.parametrize("kern", KERNELS)
def test_equal_row_and_shift_emu(emu_ctx, kern):
    _check_equal_row_and_shift(emu_ctx, kern)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNELS)
def test_equal_row_and_shift_gpu(gpu_ctx, kern):
    _check_equal_row_and_shift(gpu_ctx, kern)


# ---- the prior's edge -----------------------------------------------------------------------------------------------------------
def _check_prior_edge(ctx, kern, shape):
    D = shape["D"]
    for lnm in CC.FEED_LNM:
        for noise in CC.FEED_NOISE:
            th = np.concatenate([[np.log(1.3)], np.full(D, lnm), [np.log(noise)]])
            c = _Case(ctx, shape["N"], D, shape["M"], kern, theta=th)
            label = "%s %s ln m=%g noise=%.3g" % (kern, _sid(shape), lnm, noise)
            with _dot(ctx, -1):
                rule = [c.gp.screen_bounds(kind, par, c.eta, c.cand) for kind, par in ACQS]
                ran = c.cand.bounds_kernel()
                ratio = _mu_ratio(c, label + ", the rule")
            assert ratio <= MU_RATIO_MAX, (label, ratio)
            if lnm == -10.0:
                assert ran == DIRECT, label
                with _dot(ctx, 0):
                    off = [c.gp.screen_bounds(kind, par, c.eta, c.cand) for kind, par in ACQS]
                for (u1, l1), (u0, l0) in zip(rule, off):
                    assert _bits(u1, u0) and _bits(l1, l0), label
            _mu_ratio(c, label + ", forced")              # acq_screen_dot = 1: the per-candidate delta term carries the bounds
            assert c.cand.bounds_kernel() == DOT
            _brackets(c, label)
            c.close()


@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("shape", (dict(N=130, D=3, M=200), dict(N=257, D=8, M=200)), ids=_sid)
def test_prior_edge_emu(emu_ctx, shape, kern):
    _check_prior_edge(emu_ctx, kern, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("shape", (dict(N=130, D=3, M=200), dict(N=257, D=8, M=200)), ids=_sid)
def test_prior_edge_gpu(gpu_ctx, shape, kern):
    _check_prior_edge(gpu_ctx, kern, shape)


# ---- same answer, bit for bit ------------------------------------------------------------------------------------------------
def _argmax_only(ctx, c, kind, par, dot):
    with _dot(ctx, dot):
        c.refit()                                  # every call starts without a back-off
        out = c.gp.acq(kind, par, c.eta, c.cand, want_values=False)[1:]
        return out, c.cand.last_screen(), c.cand.bounds_kernel()


def _check_same_answer(ctx, shape, kern, default_min=False):
    c = _case(ctx, shape, kern)
    cap = max(1, c.M * 25 // 100)                  # acq_screen_keep_max = 25
    for kind, par in ACQS:
        vals, mx, am, fl = c.values(kind, par)
        with _tuned(ctx, "acq_screen", 0, None):
            off = c.gp.acq(kind, par, c.eta, c.cand, want_values=False)[1:]
        on1, (n1, kept1, out1), ran1 = _argmax_only(ctx, c, kind, par, 1)
        on0, (n0, kept0, out0), ran0 = _argmax_only(ctx, c, kind, par, 0)
        print("%s %s %s: survivors %d (dot) / %d (direct) of %d, outcomes %d / %d" % (kern, _sid(shape), kind, kept1, kept0,
                                                                                   c.M, out1, out0))
        # (a lone candidate on three block rows goes through the explicit inverse: not the screen's call under either key)
        assert n1 == n0 and n0 in (0, c.M) and (n0 > 0 or c.M == 1)
        assert n0 == 0 or (ran1, ran0) == (DOT, DIRECT)
        for on in (on1, on0):
            assert _bits([on[0]], [off[0]]) and on[1:] == off[1:], (kind, on, off)
            assert _bits([on[0]], [mx]) and on[1:] == (am, fl)
        if n0 > 0 and kept0 <= cap:                         # a condition, not a tolerance
            assert 1 <= kept1 <= cap and out1 != _lib.SCREEN_FELL_BACK, (kind, kept1, kept0, cap)


@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_same_answer_emu(emu_ctx, shape, kern):
    _check_same_answer(emu_ctx, shape, kern)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_same_answer_gpu(gpu_ctx, shape, kern):
    _check_same_answer(gpu_ctx, shape, kern)


@pytest.mark.gpu
def test_large_gpu(gpu_ctx):
    """N = 256, D = 16, M = 65 539 at the default threshold and under the rule: the dot kernel runs, the answer is the sweep's"""
    c = _Case(gpu_ctx, LARGE["N"], LARGE["D"], LARGE["M"], "matern52")
    gpu_ctx.set_tuning("acq_screen_min", None)
    try:
        vals, mx, am, fl = c.values("ei", 0.0)
        with _dot(gpu_ctx, -1):
            c.refit()
            on = c.gp.acq("ei", 0.0, c.eta, c.cand, want_values=False)[1:]
            n, kept, outcome = c.cand.last_screen()
            ran = c.cand.bounds_kernel()
        print("LARGE: survivors %d of %d, outcome %d, %s" % (kept, n, outcome, ran))
        assert ran == DOT and n == c.M and outcome == _lib.SCREEN_SCREENED and 1 <= kept <= c.M // 4
        assert _bits([on[0]], [mx]) and on[1:] == (am, fl)
    finally:
        gpu_ctx.set_tuning("acq_screen_min", 0)
        c.close()


def _check_sharded_and_multi(ctx, devices):
    shape = IDENTITY
    c = _case(ctx, shape, "matern52")
    vals, mx, am, fl = c.values("log_ei", 0.0)
    comm = _lib.Comm(ctx, 0, 1, _lib.Comm.create_id())
    try:
        with _tuned(ctx, "acq_screen", 0, None):
            off = comm.acq_sharded(c.gp, "log_ei", 0.0, c.eta, c.cand, 1000)
        kept = {}
        for dot in (1, 0):
            with _dot(ctx, dot):
                c.refit()
                on = comm.acq_sharded(c.gp, "log_ei", 0.0, c.eta, c.cand, 1000)
                kept[dot] = c.cand.last_screen()
                assert c.cand.bounds_kernel() == (DOT if dot else DIRECT)
            assert on[0] is None and _bits([on[1]], [off[1]]) and on[2:] == off[2:]
            assert _bits([on[1]], [mx]) and on[2:] == (am + 1000, 0, fl)
        print("sharded: survivors %d (dot) / %d (direct) of %d" % (kept[1][1], kept[0][1], c.M))
        if kept[0][2] == _lib.SCREEN_SCREENED:
            assert kept[1][2] == _lib.SCREEN_SCREENED
    finally:
        comm.close()
    multi = _lib.multi_for(devices)
    for mctx in multi.ctxs:
        mctx.set_tuning("acq_screen_min", 0)
    gps = [_lib.DeviceGP(mc, "matern52", shape["N"], shape["D"]) for mc in multi.ctxs]
    multi.set_data(gps, c.X, c.y)
    multi.fit(gps, c.theta, c.mean_c)
    shards = _lib.CandidateShards.split(multi.ctxs, c.Xc)
    try:
        vals, mx, am, fl = c.values("ei", 0.0)
        for mctx in multi.ctxs:
            mctx.set_tuning("acq_screen", 0)
        off = multi.acq(gps, "ei", 0.0, c.eta, shards, want_values=False)
        outcomes = {}
        for dot in (1, 0):
            for mctx in multi.ctxs:
                mctx.set_tuning("acq_screen", None)
                mctx.set_tuning("acq_screen_dot", dot)
            multi.fit(gps, c.theta, c.mean_c)
            on = multi.acq(gps, "ei", 0.0, c.eta, shards, want_values=False)
            assert _bits([on[1]], [off[1]]) and on[2:] == off[2:]
            assert _bits([on[1]], [mx]) and on[2] == am and on[4] == fl
            outcomes[dot] = [sh.last_screen() for sh in shards.shards]
            for sh in shards.shards:
                assert sh.bounds_kernel() == (DOT if dot else DIRECT)
        print("multi: survivors per shard %s (dot) / %s (direct)" % ([o[1] for o in outcomes[1]], [o[1] for o in outcomes[0]]))
        for o1, o0 in zip(outcomes[1], outcomes[0]):
            if o0[2] == _lib.SCREEN_SCREENED:
                assert o1[2] == _lib.SCREEN_SCREENED
    finally:
        for mctx in multi.ctxs:
            mctx.set_tuning("acq_screen", None)
            mctx.set_tuning("acq_screen_min", None)
            mctx.set_tuning("acq_screen_dot", None)
        if ctx in multi.ctxs:
            ctx.set_tuning("acq_screen_min", 0)
            ctx.set_tuning("acq_screen_dot", 1)
        shards.close()
        for g in gps:
            g.close()


def test_sharded_and_multi_emu(emu_ctx):
    _check_sharded_and_multi(emu_ctx, [0, 1])


@pytest.mark.gpu
def test_sharded_and_multi_gpu(gpu_ctx):
    _check_sharded_and_multi(gpu_ctx, [0, 0])


# ---- selection ----------------------------------------------------------------------------------------------------------------
def _check_selection(ctx):
    with _dot(ctx, -1):
        for name, D in (("headline", 16), ("config 2", 8)):           # N = 256 rows of the same recipe: the rule reads theta and extents
            c = _Case(ctx, 256, D, 130, "matern52")
            c.gp.screen_bounds("ei", 0.0, c.eta, c.cand)
            print("%s: %s" % (name, c.cand.bounds_kernel()))
            assert c.cand.bounds_kernel() == DOT, name
            c.close()
    for dot in (-1, 1):
        with _dot(ctx, dot):
            c = _Case(ctx, 130, 3, 130, "fabolas")
            c.gp.screen_bounds("ei", 0.0, c.eta, c.cand)
            assert c.cand.bounds_kernel() == DIRECT
            c.close()


def test_selection_emu(emu_ctx):
    _check_selection(emu_ctx)


@pytest.mark.gpu
def test_selection_gpu(gpu_ctx):
    _check_selection(gpu_ctx)
