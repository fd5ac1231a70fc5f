"""The chained small-batch solve (robo_amd/csrc/trsm_chain.hip): all block rows of the block-row substitution in ONE launch,
handing their result tiles to each other, against the launch-per-block-row form it replaces (`trsm_chain` 0 against 1).

Everything is compared bit for bit: `predict` mean and variance, the full predictive covariance, the acquisition values of a
`want_values=True` call and (max, argmax, flags) of a screened argmax-only call (`acq_screen_min` lowered to 0).
`winv_max = 0` keeps the explicit inverse out of the way; `trsm_chain_max_wg` is raised so that the interpreter's one-CU device
takes the path under the automatic rule as well.

Shapes: N in {129, 256, 257, 300, 384, 513} -- 2 to 5 block rows, n % 128 in {0, 1, 44, 127} and the skipped trailing block of
N = 256 / 384; M in {1, 16, 17, 130} -- one tile, a tile boundary, a padding-only tile next to a real one; D in {3, 16}; the
three kernels.  Inputs: bench.py's synthetic() recipe as in tests/test_acq_screen.py.

CPU: through the interpreter (tests/hipemu), which runs one workgroup at a time, i.e. in ticket order: it checks the index
arithmetic, the order of the updates and the sums, not the hand-off.  -m gpu: the same on the MI355X, plus the same comparison
with the lines of V, q and mu warm and dirty in the caches before every chained call.  The time-out path is driven in the
interpreter only, by the test-only key `trsm_chain_spin_limit = 0` (no block row publishes, the first consumer gives up at its
first poll: an early return, not a hang).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from robo_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from bench import synthetic  # noqa: E402

NS = (129, 256, 257, 300, 384, 513)
MS = (1, 16, 17, 130)
DS = (3, 16)
KERNELS = ("matern52", "rbf", "fabolas")
CHAIN, STEP = "trsm_chain_kernel", "trsm_step_small_kernel"


def _emu_lib():
    sys.path.insert(0, os.path.join(HERE, "hipemu"))
    import build_emu
    return build_emu.build()


def _tune(ctx):
    ctx.set_tuning("winv_max", 0)
    ctx.set_tuning("acq_screen_min", 0)
    ctx.set_tuning("trsm_chain_max_wg", 1 << 20)
    return ctx


@pytest.fixture(scope="module")
def emu_ctx():
    _lib.use_library(_emu_lib())
    ctx = _lib.Context(0)
    assert "hipemu" in ctx.name
    yield _tune(ctx)
    _drop(ctx)
    ctx.close()
    _lib.use_library(None)


@pytest.fixture(scope="module")
def gpu_ctx():
    _lib.use_library(None)
    if _lib.device_count() < 1:
        pytest.skip("no HIP device")
    ctx = _lib.Context(0)
    yield _tune(ctx)
    _drop(ctx)
    ctx.close()


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _inputs(N, D, M, kern):
    X, y, theta, Xc = synthetic(N, D, M, 0)
    if kern == "fabolas":
        X = np.hstack([X, np.random.RandomState(5).rand(N, 1)])
        Xc = np.hstack([Xc, np.random.RandomState(6).rand(M, 1)])
        theta = np.concatenate([theta[:-1], [np.log(0.8), np.log(1.3)], theta[-1:]])
    return X, y, theta, Xc


_GPS = {}


def _fitted(ctx, N, D, kern):
    """a fitted GP, the candidates and the incumbent: once per module and (context, shape, kernel)"""
    key = (id(ctx), N, D, kern)
    if key not in _GPS:
        X, y, theta, Xc = _inputs(N, D, max(MS), kern)
        gp = _lib.DeviceGP(ctx, kern, N, X.shape[1])
        gp.set_data(X, y)
        gp.refit = lambda: gp.fit(theta, float(np.mean(y)))
        gp.refit()
        _GPS[key] = (gp, Xc, float(y.min()))
    return _GPS[key]


def _drop(ctx):
    for key in [k for k in _GPS if k[0] == id(ctx)]:
        _GPS.pop(key)[0].close()


def _everything(ctx, gp, cand, Xm, eta, chain, warm=False):
    """-> every compared output with `trsm_chain` = chain; warm: an unchained predict on the same handle before each chained
    call, so that the lines of V, q and mu are warm and dirty in the caches when the chained kernel reads them"""
    def call(fn):
        if warm:
            ctx.set_tuning("trsm_chain", 0)
            gp.predict(cand)
        ctx.set_tuning("trsm_chain", chain)
        return fn()

    want = CHAIN if chain else STEP
    out = {}
    out["mean"], out["var"] = call(lambda: gp.predict(cand))
    assert cand.solve_kernel() == want
    out["cov_mean"], out["cov"] = call(lambda: gp.predict_cov(Xm))
    out["acq"], mx, am, fl = call(lambda: gp.acq("ei", 0.0, eta, cand, want_values=True))
    assert cand.solve_kernel() == want
    out["acq_best"] = np.array([mx, am, fl], dtype=np.float64)
    best = call(lambda: gp.acq("ei", 0.0, eta, cand, want_values=False)[1:])
    assert cand.solve_kernel() == want
    outcome = cand.last_screen()[2]
    cond = gp.factor_cond()                      # (screen.hip's conditioning guard: max L_ii / min L_ii <= 1e4)
    assert (outcome != _lib.SCREEN_NOT_ELIGIBLE) == (cond[2] <= 1e4 * cond[1]), (cand.last_screen(), cond)
    if outcome == _lib.SCREEN_FELL_BACK:         # a failed screen pauses the factor: the next screened call starts afresh
        gp.refit()
    out["screened_best"] = np.array(best, dtype=np.float64)
    return out


def _same(a, b, label):
    for key in a:
        assert _bits(a[key], b[key]), (label, key)


def _check_shape(ctx, N, D, kern, Ms=MS, repeats=1, warm=False):
    gp, Xc, eta = _fitted(ctx, N, D, kern)
    try:
        for M in Ms:
            cand = _lib.Candidates(ctx, Xc[:M])
            try:
                ref = _everything(ctx, gp, cand, Xc[:M], eta, 0)
                for _ in range(repeats):
                    _same(ref, _everything(ctx, gp, cand, Xc[:M], eta, 1, warm), (kern, N, D, M))
            finally:
                cand.close()
    finally:
        ctx.set_tuning("trsm_chain", None)


# ---- bit identity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("N", NS)
def test_bits_emu(emu_ctx, N, D, kern, M):
    _check_shape(emu_ctx, N, D, kern, Ms=(M,))


@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("N", NS)
def test_bits_gpu(gpu_ctx, N, D, kern):
    _check_shape(gpu_ctx, N, D, kern)


def _check_auto_rule(ctx):
    """-1: the chained form from three block rows on while tiles x block rows fits the bound; a bound of 0 stays on the
    launches; 1 takes two block rows as well; one block row always stays on the launches"""
    gp, Xc, _ = _fitted(ctx, 300, 3, "matern52")
    two, Xc2, _ = _fitted(ctx, 256, 3, "matern52")
    one, Xc1, _ = _fitted(ctx, 80, 3, "matern52")
    cand, cand1, cand2 = _lib.Candidates(ctx, Xc[:17]), _lib.Candidates(ctx, Xc1[:17]), _lib.Candidates(ctx, Xc2[:17])
    try:
        ctx.set_tuning("trsm_chain", -1)
        gp.predict(cand)
        assert cand.solve_kernel() == CHAIN
        two.predict(cand2)
        assert cand2.solve_kernel() == STEP
        ctx.set_tuning("trsm_chain", 1)
        two.predict(cand2)
        assert cand2.solve_kernel() == CHAIN
        ctx.set_tuning("trsm_chain", -1)
        ctx.set_tuning("trsm_chain_max_wg", 0)
        gp.predict(cand)
        assert cand.solve_kernel() == STEP
        ctx.set_tuning("trsm_chain", 1)
        one.predict(cand1)
        assert cand1.solve_kernel() == STEP
    finally:
        ctx.set_tuning("trsm_chain", None)
        ctx.set_tuning("trsm_chain_max_wg", 1 << 20)
        for h in (cand, cand1, cand2):
            h.close()


def test_auto_rule_emu(emu_ctx):
    _check_auto_rule(emu_ctx)


@pytest.mark.gpu
def test_auto_rule_gpu(gpu_ctx):
    _check_auto_rule(gpu_ctx)


# ---- work-item orders (interpreter) --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("D", DS)
def test_bits_emu_order_case(emu_ctx, D, kern):
    _check_shape(emu_ctx, 300, D, kern, Ms=(17,))


@pytest.mark.parametrize("order", ["1", "2"], ids=["descending", "rotating"])
def test_bits_in_any_work_item_order(order):
    """N = 300, M = 17 again with the work-items of a workgroup run in descending and in rotating order"""
    _emu_lib()
    e = dict(os.environ, ROBO_TESTS_SERIAL="1", HIPEMU_ORDER=order)
    e["PYTHONPATH"] = os.pathsep.join([os.path.dirname(HERE), e.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-p", "no:cacheprovider",
                        "-k", "emu_order_case"], env=e, cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout


# ---- dirty lines (MI355X) ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kern", KERNELS)
def test_bits_with_warm_dirty_lines_gpu(gpu_ctx, kern):
    """an unchained predict on the same handle before every chained call leaves the lines of V, q and mu warm and dirty; three
    chained passes on one handle, each compared"""
    _check_shape(gpu_ctx, 513, 16, kern, Ms=(17, 130), repeats=3, warm=True)


# ---- the time-out path (interpreter only) --------------------------------------------------------------------------------------
def test_time_out_falls_back_to_the_launches(emu_ctx):
    """`trsm_chain_spin_limit = 0`: no block row publishes and a consumer gives up at its first unsuccessful poll, so block
    row 1 of every tile waits once and returns.  The call still answers with the launches' bits, the context stays off the
    chain, and the message can be read."""
    ctx = _tune(_lib.Context(0))
    gp, Xc, eta = _fitted(ctx, 300, 3, "matern52")
    cand = _lib.Candidates(ctx, Xc[:17])
    try:
        ctx.set_tuning("trsm_chain", 0)
        ref = gp.predict(cand)
        ref_acq = gp.acq("ei", 0.0, eta, cand, want_values=True)
        ref_cov = gp.predict_cov(Xc[:17])
        for fn, want, on_cand in ((lambda: gp.predict(cand), ref, True),
                                  (lambda: gp.acq("ei", 0.0, eta, cand, want_values=True), ref_acq, True),
                                  (lambda: gp.predict_cov(Xc[:17]), ref_cov, False)):      # (a handle of its own)
            ctx.set_tuning("trsm_chain", 1)              # (re-arms the context)
            ctx.set_tuning("trsm_chain_spin_limit", 0)
            got = fn()
            assert len(got) == len(want)
            for a, b in zip(got, want):
                assert _bits(a, b)
            if on_cand:
                assert cand.solve_kernel() == STEP
            assert "trsm_chain_kernel" in _lib.last_error() and "launches" in _lib.last_error()
            # the context stays off the chain, whatever the spin limit says now
            ctx.set_tuning("trsm_chain_spin_limit", None)
            mu, var = gp.predict(cand)
            assert cand.solve_kernel() == STEP and _bits(mu, ref[0]) and _bits(var, ref[1])
        ctx.set_tuning("trsm_chain", 1)                  # re-armed: the chained kernel again, the same bits
        mu, var = gp.predict(cand)
        assert cand.solve_kernel() == CHAIN and _bits(mu, ref[0]) and _bits(var, ref[1])
    finally:
        cand.close()
        _drop(ctx)
        ctx.close()
