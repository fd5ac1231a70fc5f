"""Device-resident multi-start gradient refinement of an acquisition maximum (robo_amd/csrc/refine.hip,
robo_acq_refine_cand / robo_acq_refine_marginal_cand, ClosedFormAcquisition.refine, DeviceGradientAscent) against the
fp64 oracle through tests/refine_oracle.py.

Whole trajectories are not compared: a rounding-level difference may flip one accept test and send two correct
trajectories apart.  Instead every step of the device's trace is checked on its own -- value and gradient against the
oracle at the device's own trial point, the trial point, the accept bit and the step length against the rule applied to
the device's own stored doubles.
CPU: through the interpreter (tests/hipemu), small sizes.  -m gpu: the MI355X at N = 4096, D = 16, 65 536 candidates,
256 starts, 50 steps.
"""
import os
import sys

import numpy as np
import pytest

from robo_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refine_oracle as RO  # noqa: E402
from _tol import ACQ_RTOL, assert_logei_close  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402

G_RTOL, G_ATOL_REL = 1e-7, 1e-8        # the figures check_predictive_gradients holds the variance gradient to
SMALL = dict(N=80, D=3, M=400, K=6, T=8)
LARGE = dict(N=4096, D=16, M=65536, K=256, T=50)
ACQS = (("ei", 0.0), ("log_ei", 0.0), ("pi", 0.0), ("lcb", 1.0))


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
def _theta(D, ls2, noise=1e-2, kind="matern52"):
    if kind == "fabolas":            # D - 1 configuration columns + the fidelity column with its two regression parameters
        ls2 = ls2 if np.ndim(ls2) == 0 else np.asarray(ls2)[:D - 1]
        return np.concatenate([[0.0], np.log(np.broadcast_to(ls2, (D - 1,))), [np.log(0.5), np.log(0.8)], [np.log(noise)]])
    return np.concatenate([[0.0], np.log(np.broadcast_to(ls2, (D,))), [np.log(noise)]])


def _data(N, D, seed):
    rs = np.random.RandomState(seed)
    X = rs.rand(N, D)
    y = np.sin(3 * X.sum(axis=1) / np.sqrt(D / 3.0)) + 0.1 * rs.randn(N)
    return rs, X, y


def _pair(ctx, kind, theta, X, y):
    """the same GP as oracle and on the device (inputs already in [0, 1]^D)"""
    ogp = O.OracleGP(kind, theta, normalize_input=False)
    ogp.train(X, y)
    g = _lib.DeviceGP(ctx, kind, X.shape[0], X.shape[1])
    g.set_data(X, y)
    g.fit(theta, ogp.mean)
    return ogp, g


def _setup(ctx, sz, kernel="matern52", seed=0):
    D = sz["D"]
    rs, X, y = _data(sz["N"], D, seed)
    ls2 = np.array([0.3, 0.5, 0.8, 0.4, 0.6])[:D] if D <= 5 else 0.25 * D
    ogp, g = _pair(ctx, kernel, _theta(D, ls2, kind=kernel), X, y)
    return rs, ogp, g, y, rs.rand(sz["M"], D)


def _replay(trace, starts, step0, floored=None):
    """every (t, k) of a trace against the rule, on the device's own doubles -> (f at the start, final f, final x);
    floored(y) -> bool, if given: does the oracle's variance sit on its floor at y (the only input of a decision that
    the trace does not carry; code 3 marks it)"""
    T1, K, W = trace.shape
    D = (W - 3) // 2
    f0, fT, xT = np.full(K, -np.inf), np.full(K, -np.inf), np.zeros((K, D))
    steps = 0
    for k in range(K):
        if starts[k] < 0:
            assert np.all(trace[:, k, -1] == 2)
            continue
        x, f, g = trace[0, k, :D].copy(), trace[0, k, D], trace[0, k, D + 1:2 * D + 1].copy()
        assert trace[0, k, -1] in (1, 3) and trace[0, k, 2 * D + 1] == step0
        assert np.isfinite(f) or trace[0, k, -1] == 3
        alpha, frozen = step0, trace[0, k, -1] == 3      # 3: variance on its floor or value not finite at the start
        f0[k] = f
        for t in range(1, T1):
            y, fy, gy, a_used, code = trace[t, k, :D], trace[t, k, D], trace[t, k, D + 1:2 * D + 1], \
                trace[t, k, 2 * D + 1], trace[t, k, -1]
            assert np.all((y >= 0.0) & (y <= 1.0))
            steps += 1
            want, stop = RO.trial_point(x, g, alpha)
            if frozen or stop:
                frozen = True
                assert code == 2 and np.array_equal(y, x), (t, k)
                continue
            assert code in (0, 1, 3) and a_used == alpha, (t, k, code, a_used, alpha)
            assert np.all(np.abs(y - want) <= 4 * np.spacing(np.maximum(np.abs(x), np.abs(want)))), (t, k, y, want)
            if floored is not None:
                assert (code == 3) == bool(floored(y) or not np.isfinite(fy)), (t, k, code, fy)
            if code == 3 or not np.isfinite(fy):       # the trial is not taken and the start stops
                assert code == 3
                frozen = True
                continue
            assert code == (1 if fy > f else 0), (t, k, fy, f, code)
            if fy > f:
                x, f, g, alpha = y.copy(), fy, gy.copy(), min(2.0 * alpha, 0.5)
            else:
                alpha = alpha / 2.0
        fT[k], xT[k] = f, x
    assert steps == int((starts >= 0).sum()) * (T1 - 1)          # no step left out
    return f0, fT, xT


def _against_oracle(trace, starts, ogps, kind, par, etas, label=""):
    """value and gradient of every trace entry against the oracle at the device's own trial point"""
    T1, K, W = trace.shape
    D = (W - 3) // 2
    used = starts >= 0
    P = trace[:, used, :D].reshape(-1, D)
    fd = trace[:, used, D].ravel()
    gd = trace[:, used, D + 1:2 * D + 1].reshape(-1, D)
    fo, go = RO.evaluator(ogps, kind, par, etas)(P)
    gmax = np.abs(go).max()
    with np.errstate(divide="ignore", invalid="ignore"):
        print("%s %s: %d points, max rel value error %.3e, max gradient error / max|g| %.3e, max rel gradient error %.3e"
              % (label, kind, P.shape[0], np.nanmax(np.abs(fd - fo) / np.abs(fo)), np.abs(gd - go).max() / gmax,
                 np.nanmax(np.abs(gd - go) / np.maximum(np.abs(go), G_ATOL_REL * gmax / G_RTOL))))
    if kind == "log_ei" and len(ogps) == 1:
        assert_logei_close(fd, fo, RO.z_of(ogps[0], par, np.ravel(etas)[0], P), rtol=ACQ_RTOL, tail_rtol=ACQ_RTOL)
    else:
        np.testing.assert_allclose(fd, fo, rtol=ACQ_RTOL, atol=0)
    np.testing.assert_allclose(gd, go, rtol=G_RTOL, atol=G_ATOL_REL * gmax)


def _result_checks(r, trace_f, xT, starts):
    f0, fT = trace_f
    used = starts >= 0
    assert np.all(fT[used] >= f0[used])
    best = int(np.argmax(np.where(used, fT, -np.inf)))
    assert r.value == fT[best] and r.start_index == starts[best]
    np.testing.assert_array_equal(r.x, xT[best])


# ---- 1. the oracle's gradients (pure CPU) ----------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["matern52", "rbf", "fabolas"])
def test_oracle_gradients_against_central_differences(kernel):
    rs, X, y = _data(70, 3, 5)
    ogp = O.OracleGP(kernel, _theta(3, [0.3, 0.5, 0.8], kind=kernel), normalize_input=False)
    ogp.train(X, y)
    P = 0.05 + 0.9 * rs.rand(40, 3)
    m, v, dm, dv = RO.moments(ogp, P)
    dmo, dvo = ogp.predictive_gradients(P)
    np.testing.assert_allclose(dm, dmo[:, :, 0], rtol=1e-11, atol=1e-13)     # the blocked form = the oracle's loop
    np.testing.assert_allclose(dv, dvo, rtol=1e-11, atol=1e-13)
    h = 1e-5
    seen = []
    for kind, par in ACQS:
        # incumbents that put z = (eta - m - par) / s over [-8, 3]
        for zt in (-8.0, -4.0, -1.0, 1.0, 3.0):
            eta = float(np.median(m + zt * np.sqrt(v)))
            z = (eta - m - par) / np.sqrt(v)
            keep = (z >= -8.0) & (z <= 3.0)
            seen.append(z[keep])
            fn = RO.evaluator([ogp], kind, par, eta)
            _, g = fn(P[keep])
            for d in range(3):
                e = np.zeros(3)
                e[d] = h
                num = (fn(P[keep] + e)[0] - fn(P[keep] - e)[0]) / (2 * h)
                np.testing.assert_allclose(g[:, d], num, rtol=1e-5, atol=1e-6 * max(1.0, np.abs(g).max()))
    seen = np.concatenate(seen)
    assert seen.min() < -7.0 and seen.max() > 2.5


def test_logei_ratio_in_the_tail():
    """Phi / h: erfcx core and asymptotic series against the cancellation-free continued fraction in extended
    precision, across the switch point and down to z = -1e3; continuity at the two switches"""
    z = -np.concatenate([np.linspace(1.0, 40.0, 400), np.logspace(np.log10(40.0), 3.0, 60),
                         [RO.TAIL_T, np.nextafter(RO.TAIL_T, 0.0), np.nextafter(RO.TAIL_T, 100.0)]])
    got = RO.cdf_over_h(z)
    ref = RO.cdf_over_h_reference(z).astype(np.float64)
    err = np.abs(got - ref) / ref
    t = -z
    print("max rel error: core (t < 16) %.2e, series (t >= 16) %.2e" % (err[t < RO.TAIL_T].max(), err[t >= RO.TAIL_T].max()))
    assert np.all(err[t < RO.TAIL_T] <= 4 * t[t < RO.TAIL_T] ** 2 * np.finfo(float).eps + 1e-15)   # eps t^2 amplification
    assert np.all(err[t >= RO.TAIL_T] <= 8 * np.finfo(float).eps)
    a, b = RO.cdf_over_h(np.array([-1.0, np.nextafter(-1.0, -2.0)]))
    assert abs(a - b) <= 1e-14 * a


# ---- 2. selection -----------------------------------------------------------------------------------------------------
def _check_selection(ctx, sz):
    rs, ogp, g, y, Xc = _setup(ctx, sz)
    K, D = sz["K"], sz["D"]
    Xc[7] = Xc[3]                                   # duplicated candidates: ties
    Xc[11] = Xc[3]
    Xc[sz["M"] // 2:sz["M"] // 2 + 5] = Xc[3]
    cand = _lib.Candidates(ctx, Xc)
    try:
        for kind, par in ACQS:
            vals, mx, am, _ = g.acq(kind, par, y.min(), cand)
            r = g.refine(kind, par, y.min(), cand, K, 0, 0.05, diagnostics=True)
            np.testing.assert_array_equal(r.starts, np.argsort(-vals, kind="stable")[:K])
            assert r.start_index == am and r.value == mx            # T = 0: the sweep's own answer, bit for bit
            np.testing.assert_array_equal(r.x, Xc[am])
        # everything tied: the first K rows
        flat = _lib.Candidates(ctx, np.tile(Xc[3], (sz["M"], 1)))
        r = g.refine("lcb", 1.0, 0.0, flat, K, 0, 0.05, diagnostics=True)
        np.testing.assert_array_equal(r.starts, np.arange(K))
        flat.close()
    finally:
        cand.close()
    # NaN rows are never selected; fewer eligible rows than K: K shrinks
    Xn = rs.rand(12, D)
    Xn[[0, 2, 3, 5, 8, 9, 11], 0] = np.nan
    few = _lib.Candidates(ctx, Xn)
    try:
        vals, _, _, fl = g.acq("lcb", 1.0, 0.0, few)
        assert np.isnan(vals).sum() == 7 and fl & _lib.FLAG_NAN
        for K2 in (3, 8):
            r = g.refine("lcb", 1.0, 0.0, few, K2, 2, 0.05, diagnostics=True)
            order = np.argsort(-vals, kind="stable")
            order = order[~np.isnan(vals[order])][:K2]
            want = np.full(K2, -1)
            want[:len(order)] = order
            np.testing.assert_array_equal(r.starts, want)
            assert r.flags & _lib.FLAG_NAN and np.isfinite(r.value) and np.all(np.isfinite(r.x))
            assert r.start_index in order
    finally:
        few.close()
        g.close()


def test_selection(emu_ctx):
    _check_selection(emu_ctx, SMALL)


@pytest.mark.gpu
def test_selection_gpu(gpu_ctx):
    _check_selection(gpu_ctx, LARGE)


# ---- 3. + 4. every step on its own; properties -------------------------------------------------------------------------
def _check_steps(ctx, sz, kernel, acqs, label):
    rs, ogp, g, y, Xc = _setup(ctx, sz, kernel)
    K, T = sz["K"], sz["T"]
    cand = _lib.Candidates(ctx, Xc)
    try:
        for kind, par in acqs:
            eta = float(y.min())
            r = g.refine(kind, par, eta, cand, K, T, 0.05, diagnostics=True)
            assert r.trace.shape == (T + 1, K, 2 * sz["D"] + 3) and np.all(r.starts >= 0)
            f0, fT, xT = _replay(r.trace, r.starts, 0.05)
            _result_checks(r, (f0, fT), xT, r.starts)
            _against_oracle(r.trace, r.starts, [ogp], kind, par, eta, label + " " + kernel)
            _, mx, _, _ = g.acq(kind, par, eta, cand, want_values=False)
            assert r.value >= mx - ACQ_RTOL * abs(mx)          # (the sweep and the gradient path round differently)
            # the same call without diagnostics: the same answer
            r2 = g.refine(kind, par, eta, cand, K, T, 0.05)
            assert r2.value == r.value and r2.start_index == r.start_index and np.array_equal(r2.x, r.x)
    finally:
        cand.close()
        g.close()


@pytest.mark.parametrize("kernel", ["matern52", "rbf"])
def test_every_step(emu_ctx, kernel):
    _check_steps(emu_ctx, SMALL, kernel, ACQS, "interpreter")


def test_every_step_fabolas_kernel(emu_ctx):
    _check_steps(emu_ctx, dict(N=140, D=4, M=300, K=5, T=6), "fabolas", ACQS, "interpreter")


def test_every_step_through_the_explicit_inverse(emu_ctx):
    """factors that qualify for W = L^-1 (from six block rows on by default; here from two) take the triangular product
    instead of the block-row substitution: the same checks, the same answers to rounding, and the same bits whatever
    the number of starts (the product runs in the one form whose association does not depend on the row count)"""
    sz = dict(N=300, D=3, M=300, K=5, T=5)
    acqs = (("log_ei", 0.0), ("lcb", 1.0))

    def traces():
        rs, ogp, g, y, Xc = _setup(emu_ctx, sz)
        cand = _lib.Candidates(emu_ctx, Xc)
        try:
            return [g.refine(kind, par, y.min(), cand, K, sz["T"], 0.05, diagnostics=True).trace
                    for kind, par in acqs for K in (5, 12)]
        finally:
            cand.close()
            g.close()
    plain = traces()
    emu_ctx.set_tuning("winv_min_blocks", 2)
    try:
        _check_steps(emu_ctx, sz, "matern52", acqs, "interpreter, W")
        through_w = traces()
    finally:
        emu_ctx.set_tuning("winv_min_blocks", None)
    for a, b in zip(plain, through_w):
        assert not np.array_equal(a[0], b[0])                                 # another solve: other roundings
        np.testing.assert_allclose(a[0, :, :-2], b[0, :, :-2], rtol=1e-9, atol=1e-12)
    for i in (0, 2):
        np.testing.assert_array_equal(through_w[i], through_w[i + 1][:, :5])


@pytest.mark.gpu
def test_every_step_gpu(gpu_ctx):
    _check_steps(gpu_ctx, LARGE, "matern52", (("log_ei", 0.0),), "MI355X")


@pytest.mark.gpu
def test_every_step_other_acquisitions_at_full_size_gpu(gpu_ctx):
    """EI, PI and LCB at N = 4096, D = 16, 65 536 candidates, 256 starts, but 4 steps instead of 50: the oracle costs
    about a second per thousand N = 4096 predictions with gradients on the host, and everything that depends on N -- the solve and the dot
    products -- is shared with the 50-step LogEI run above; only the epilogue's formulas differ"""
    _check_steps(gpu_ctx, dict(LARGE, T=4), "matern52", (("ei", 0.0), ("pi", 0.0), ("lcb", 1.0)), "MI355X")


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["matern52", "rbf", "fabolas"])
def test_every_step_all_acquisitions_gpu(gpu_ctx, kernel):
    _check_steps(gpu_ctx, dict(N=300, D=5, M=2000, K=16, T=12), kernel, ACQS, "MI355X small")


def _check_face_and_underflow(ctx):
    # the maximum of this problem lies on the face x_1 = 1: starts on that face keep x_1 = 1 while the gradient points out
    rs, X, y = _data(60, 2, 0)
    ogp, g = _pair(ctx, "matern52", _theta(2, [0.3, 0.5]), X, y)
    Xc = rs.rand(300, 2)
    Xc[:, 1] = 1.0
    cand = _lib.Candidates(ctx, Xc)
    try:
        r = g.refine("lcb", 1.0, 0.0, cand, 6, 10, 0.05, diagnostics=True)
        f0, fT, xT = _replay(r.trace, r.starts, 0.05)
        _result_checks(r, (f0, fT), xT, r.starts)
        out = r.trace[:, :, 2 + 1 + 1] > 0                              # d f / d x_1 at every trial
        assert out[0].any()
        assert out.all(axis=0).any()                                    # some start is pushed outward all the way
        for k in range(6):
            if out[:, k].all():
                assert np.all(r.trace[:, k, 1] == 1.0)
        # and step by step: from a point on the face whose gradient points out, the next trial is on the face
        for k in range(6):
            xk, gk = r.trace[0, k, :2], r.trace[0, k, 3:5]
            for t in range(1, 11):
                if r.trace[t, k, -1] == 2:
                    break
                if xk[1] == 1.0 and gk[1] > 0:
                    assert r.trace[t, k, 1] == 1.0
                if r.trace[t, k, -1] == 1:
                    xk, gk = r.trace[t, k, :2], r.trace[t, k, 3:5]
        assert r.x[1] == 1.0 and r.value > f0.max()
        # EI with an incumbent 1000 below every prediction: Phi = phi = 0, EI = 0 and its gradient vanish everywhere
        vals, mx, am, _ = g.acq("ei", 0.0, y.min() - 1e3, cand)
        assert np.all(vals == 0.0)
        r = g.refine("ei", 0.0, y.min() - 1e3, cand, 6, 5, 0.05, diagnostics=True)
        assert r.flags & _lib.FLAG_FROZEN and not r.flags & _lib.FLAG_NAN
        assert r.value == 0.0 and r.start_index == am == 0 and np.array_equal(r.x, Xc[0])
        assert np.all(np.isfinite(r.trace)) and np.all(r.trace[1:, :, -1] == 2)
        _replay(r.trace, r.starts, 0.05)
    finally:
        cand.close()
        g.close()


def _check_logei_tail(ctx, sz):
    """incumbents far below the data drive z = (eta - m) / s through both tail branches of Phi / h on the device: the
    erfcx core (1 < -z < 16), the asymptotic series (-z >= 16) and the switch between them"""
    rs, ogp, g, y, Xc = _setup(ctx, sz)
    cand = _lib.Candidates(ctx, Xc)
    zs = []
    try:
        for off in (1.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 10.0, 14.0, 17.0, 30.0, 200.0):
            eta = float(y.min() - off)
            r = g.refine("log_ei", 0.0, eta, cand, sz["K"], sz["T"], 0.05, diagnostics=True)
            _replay(r.trace, r.starts, 0.05)
            _against_oracle(r.trace, r.starts, [ogp], "log_ei", 0.0, eta, "tail, eta = min - %g" % off)
            zs.append(RO.z_of(ogp, 0.0, eta, r.trace[:, :, :sz["D"]].reshape(-1, sz["D"])))
    finally:
        cand.close()
        g.close()
    z = np.concatenate(zs)
    print("z from %.1f to %.1f" % (z.min(), z.max()))
    assert ((z < -1.0) & (z > -RO.TAIL_T)).sum() >= 20 and (z <= -RO.TAIL_T).sum() >= 20 and z.min() < -500.0
    assert ((z < -12.0) & (z > -RO.TAIL_T)).any() and ((z <= -RO.TAIL_T) & (z > -20.0)).any()     # both sides of the switch


def test_logei_tail_on_the_device(emu_ctx):
    _check_logei_tail(emu_ctx, SMALL)


@pytest.mark.gpu
def test_logei_tail_on_the_device_gpu(gpu_ctx):
    _check_logei_tail(gpu_ctx, dict(LARGE, K=64, T=3))


def _check_variance_floor(ctx):
    """an output scale of 1e-4 puts the variance at the training points (~1e-8 before scaling) below the floor of 2.2e-16:
    starts there are marked 3 at once and stay; a trial that lands on the floor later is not taken, whatever its value"""
    rs, X, y = _data(60, 2, 1)
    theta = _theta(2, [0.3, 0.5], noise=1e-8)
    ogp, g = _pair(ctx, "matern52", theta, X, y)
    g.set_output_transform(0.0, 1e-4)

    def floored(p):
        return ogp.predict(np.atleast_2d(p), diag_only=True)[1][0] * 1e-8 < np.finfo(float).eps
    Xc = np.vstack([X[:4], rs.rand(8, 2), X[4:9] + 1e-3])
    assert all(floored(p) for p in Xc[:4]) and not any(floored(p) for p in Xc[4:12])
    cand = _lib.Candidates(ctx, Xc)
    try:
        for kind, par in (("lcb", 1.0), ("log_ei", 0.0)):
            r = g.refine(kind, par, float(y.min() * 1e-4), cand, len(Xc), 12, 0.05, diagnostics=True)
            f0, fT, xT = _replay(r.trace, r.starts, 0.05, floored)
            on_data = np.isin(r.starts, np.arange(4))
            assert on_data.sum() == 4
            assert np.all(r.trace[0, on_data, -1] == 3) and np.all(r.trace[1:, on_data, -1] == 2)
            at_start = np.array([floored(p) for p in Xc[r.starts]])
            np.testing.assert_array_equal(r.trace[0, :, -1], np.where(at_start, 3, 1))
            assert not at_start[np.isin(r.starts, np.arange(4, 12))].any()
            assert r.flags & _lib.FLAG_FROZEN and np.isfinite(r.value)
            print("%s: codes %s" % (kind, dict(zip(*np.unique(r.trace[:, :, -1], return_counts=True)))))
    finally:
        cand.close()
        g.close()


def test_variance_floor(emu_ctx):
    _check_variance_floor(emu_ctx)


@pytest.mark.gpu
def test_variance_floor_gpu(gpu_ctx):
    _check_variance_floor(gpu_ctx)


def test_face_and_underflow(emu_ctx):
    _check_face_and_underflow(emu_ctx)


@pytest.mark.gpu
def test_face_and_underflow_gpu(gpu_ctx):
    _check_face_and_underflow(gpu_ctx)


def test_arguments(emu_ctx):
    rs, ogp, g, y, Xc = _setup(emu_ctx, SMALL)
    cand = _lib.Candidates(emu_ctx, Xc)
    other = _lib.Candidates(emu_ctx, rs.rand(10, 2))
    fresh = _lib.DeviceGP(emu_ctx, "matern52", 80, 3)
    try:
        for K, T, s0 in ((0, 3, 0.05), (1025, 3, 0.05), (4, -1, 0.05), (4, 3, 0.0), (4, 3, np.nan)):
            with pytest.raises(ValueError):
                g.refine("lcb", 1.0, 0.0, cand, K, T, s0)
        with pytest.raises(_lib.RoboBadShape):
            g.refine("lcb", 1.0, 0.0, other, 4, 3, 0.05)
        with pytest.raises(Exception, match="trained first"):
            fresh.refine("lcb", 1.0, 0.0, cand, 4, 3, 0.05)
        assert g.refine("lcb", 1.0, 0.0, cand, 4, 3, 0.05).flags == 0      # the handle is still usable
    finally:
        for h in (cand, other, fresh, g):
            h.close()


# ---- 5. it finds what the candidates miss ------------------------------------------------------------------------------
def _dense_optimum(fn):
    from scipy import optimize
    g1 = np.linspace(0.0, 1.0, 201)
    G = np.array(np.meshgrid(g1, g1)).reshape(2, -1).T
    x0 = G[np.argmax(fn(G)[0])]
    res = optimize.minimize(lambda x: tuple(-v[0] for v in fn(x[None, :])), x0, jac=True, method="L-BFGS-B",
                            bounds=[(0.0, 1.0)] * 2, options=dict(ftol=1e-15, gtol=1e-12))
    return res.x, -res.fun


def _check_closes_the_gap(ctx):
    """N = 60, D = 2, 300 candidates, 8 starts, 60 steps, data seed 8: the maxima of LCB and LogEI are interior (both
    near (0.751, 0.518)); the NumPy restatement alone leaves 1.5e-9 / 5.9e-10 of the gap between the sweep's best and
    the optimum, so the bound of 0.01 leaves the device's rounding-level differences ample room."""
    rs, X, y = _data(60, 2, 8)
    ogp, g = _pair(ctx, "matern52", _theta(2, [0.3, 0.5]), X, y)
    Xc = rs.rand(300, 2)
    cand = _lib.Candidates(ctx, Xc)
    try:
        for kind, par in (("lcb", 1.0), ("log_ei", 0.0)):
            eta = float(y.min())
            fn = RO.evaluator([ogp], kind, par, eta)
            x_star, f_star = _dense_optimum(fn)
            assert np.all((x_star > 0.0) & (x_star < 1.0))
            sweep = fn(Xc)[0]
            host = RO.refine(fn, sweep, Xc, 8, 60)
            assert f_star - host["value"] <= 1e-3 * (f_star - sweep.max())
            _, mx, _, _ = g.acq(kind, par, eta, cand, want_values=False)
            r = g.refine(kind, par, eta, cand, 8, 60, 0.05)
            print("%s: f* %.15g sweep %.15g refined %.15g, gap left %.3e" % (kind, f_star, mx, r.value,
                                                                              (f_star - r.value) / (f_star - mx)))
            assert r.value > mx
            assert f_star - r.value <= 0.01 * (f_star - mx)
            assert np.abs(fn(r.x[None, :])[0][0] - r.value) <= ACQ_RTOL * abs(r.value)
    finally:
        cand.close()
        g.close()


def test_closes_the_gap(emu_ctx):
    _check_closes_the_gap(emu_ctx)


@pytest.mark.gpu
def test_closes_the_gap_gpu(gpu_ctx):
    _check_closes_the_gap(gpu_ctx)


# ---- 6. marginal form -----------------------------------------------------------------------------------------------------
def _check_marginal(ctx, sz, acqs=(("log_ei", 0.0), ("lcb", 1.0), ("ei", 0.01))):
    D, K, T = sz["D"], sz["K"], sz["T"]
    rs, X, y = _data(sz["N"], D, 3)
    base = np.array([0.3, 0.5, 0.8, 0.4, 0.6])[:D] if D <= 5 else np.full(D, 0.25 * D)
    pairs = [_pair(ctx, "matern52", _theta(D, base * f), X, y) for f in (1.0, 0.6, 1.7)]
    ogps, gps = [p[0] for p in pairs], [p[1] for p in pairs]
    cand = _lib.Candidates(ctx, rs.rand(sz["M"], D))
    etas = np.array([y.min(), y.min() - 0.05, y.min() + 0.02])
    try:
        for kind, par in acqs:
            vals, mx, am, _ = _lib.acq_marginal(gps, kind, par, etas, cand)
            r = _lib.acq_refine(gps, kind, par, etas, cand, K, T, 0.05, diagnostics=True)
            np.testing.assert_array_equal(r.starts, np.argsort(-vals, kind="stable")[:K])
            f0, fT, xT = _replay(r.trace, r.starts, 0.05)
            _result_checks(r, (f0, fT), xT, r.starts)
            _against_oracle(r.trace, r.starts, ogps, kind, par, etas, "marginal S=3")
            r0 = _lib.acq_refine(gps, kind, par, etas, cand, K, 0, 0.05)
            assert r0.value == mx and r0.start_index == am
            # one sample: the marginal entry point is the single-GP one, bit for bit
            a = _lib.acq_refine(gps[1:2], kind, par, etas[1:2], cand, K, T, 0.05, diagnostics=True)
            b = gps[1].refine(kind, par, etas[1], cand, K, T, 0.05, diagnostics=True)
            np.testing.assert_array_equal(a.trace, b.trace)
            np.testing.assert_array_equal(a.starts, b.starts)
            assert a.value == b.value and a.start_index == b.start_index and a.flags == b.flags
            np.testing.assert_array_equal(a.x, b.x)
    finally:
        cand.close()
        for g in gps:
            g.close()


def test_marginal(emu_ctx):
    _check_marginal(emu_ctx, dict(N=80, D=3, M=300, K=4, T=5))


@pytest.mark.gpu
def test_marginal_gpu(gpu_ctx):
    # LogEI with all 50 steps; LCB and EI with 6 (three oracle GPs per trial point: see the note on the 4-step run above)
    _check_marginal(gpu_ctx, LARGE, (("log_ei", 0.0),))
    _check_marginal(gpu_ctx, dict(LARGE, T=6), (("lcb", 1.0), ("ei", 0.01)))


# ---- 7. independence --------------------------------------------------------------------------------------------------------
def _check_independence(ctx, sz, ks):
    rs, ogp, g, y, Xc = _setup(ctx, sz, seed=4)
    cand = _lib.Candidates(ctx, Xc)
    try:
        for kind, par in (("log_ei", 0.0), ("lcb", 1.0)):
            a = g.refine(kind, par, y.min(), cand, ks[0], sz["T"], 0.05, diagnostics=True)
            b = g.refine(kind, par, y.min(), cand, ks[1], sz["T"], 0.05, diagnostics=True)
            np.testing.assert_array_equal(a.starts, b.starts[:ks[0]])
            np.testing.assert_array_equal(a.trace, b.trace[:, :ks[0]])
            again = g.refine(kind, par, y.min(), cand, ks[1], sz["T"], 0.05, diagnostics=True)
            np.testing.assert_array_equal(again.trace, b.trace)
    finally:
        cand.close()
        g.close()


def _check_shape_change(ctx):
    """one live handle through the state-block shapes 3 starts -> 8 starts -> 3 starts: every reallocation gives the bits
    of a handle that never held another shape (N = 22, D = 2, 40 candidates, 2 steps: every array of the block is
    non-empty and the odd counts make the 16-byte round-up between the arrays matter)"""
    sz = dict(N=22, D=2, M=40)
    (_, _, live, y, Xc), (_, _, fresh, _, _) = _setup(ctx, sz, seed=5), _setup(ctx, sz, seed=5)
    cand = _lib.Candidates(ctx, Xc)

    def run(g, k):
        return g.refine("log_ei", 0.0, y.min(), cand, k, 2, 0.05, diagnostics=True)

    try:
        first, more, again = run(live, 3), run(live, 8), run(live, 3)
        for a, b in ((first, again), (more, run(fresh, 8))):
            assert (a.start_index, a.flags) == (b.start_index, b.flags)
            for p, r in ((a.x, b.x), (np.float64(a.value), np.float64(b.value)), (a.starts, b.starts), (a.trace, b.trace)):
                assert p.tobytes() == r.tobytes()
    finally:
        cand.close()
        live.close()
        fresh.close()


def test_independence(emu_ctx):
    _check_independence(emu_ctx, SMALL, (4, 16))
    _check_shape_change(emu_ctx)


@pytest.mark.gpu
def test_independence_gpu(gpu_ctx):
    _check_independence(gpu_ctx, LARGE, (4, 16))
    _check_independence(gpu_ctx, dict(LARGE, T=10), (64, 256))
    _check_shape_change(gpu_ctx)


# ---- 8. classes and front end --------------------------------------------------------------------------------------------------
def _branin(x):
    a, b, c, r, s, t = 1.0, 5.1 / (4 * np.pi ** 2), 5.0 / np.pi, 6.0, 10.0, 1.0 / (8 * np.pi)
    return float(a * (x[1] - b * x[0] ** 2 + c * x[0] - r) ** 2 + s * (1 - t) * np.cos(x[0]) + s)


BRANIN_LO, BRANIN_HI = np.array([-5.0, 0.0]), np.array([10.0, 15.0])


def _check_classes(ctx):
    from robo_amd.acquisition_functions import EI, LCB, LogEI, MarginalizationGPMCMC, PI
    from robo_amd.acquisition_functions.base_acquisition import BaseAcquisitionFunction
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.maximizers import DeviceGradientAscent
    from robo_amd.models import GaussianProcess
    rs = np.random.RandomState(0)
    X = BRANIN_LO + (BRANIN_HI - BRANIN_LO) * rs.rand(12, 2)
    y = np.array([_branin(x) for x in X])

    def model(scale, **kw):
        m = GaussianProcess(2 * Matern52Kernel(np.full(2, scale), ndim=2), noise=1e-3, lower=BRANIN_LO, upper=BRANIN_HI,
                            rng=np.random.RandomState(3), **kw)
        m.train(X, y, do_optimize=False)
        return m
    m = model(0.3)
    Xc = BRANIN_LO + (BRANIN_HI - BRANIN_LO) * rs.rand(200, 2)
    for cls in (EI, LogEI, PI, LCB):
        a = cls(m)
        x = a.refine(Xc, n_starts=4, n_steps=6)
        assert x.shape == (2,) and np.all(x >= BRANIN_LO) and np.all(x <= BRANIN_HI)
        best = Xc[a.argmax(Xc)]
        assert a.compute(x[None, :])[0] >= a.compute(best[None, :])[0] * (1 - 1e-9 * np.sign(a.compute(best[None, :])[0]))
        np.testing.assert_array_equal(a.refine(Xc, n_starts=4, n_steps=0), best)
        assert a.last_refine.start_index == a.last_argmax
    # marginalised over sub-models

    class Mix(object):
        def __init__(self, models):
            self.models = models

        def get_incumbent(self):
            return self.models[0].get_incumbent()
    mix = Mix([model(0.3), model(0.2), model(0.5)])
    acq = MarginalizationGPMCMC(LogEI(mix))
    x = acq.refine(Xc, n_starts=4, n_steps=6)
    assert np.all(x >= BRANIN_LO) and np.all(x <= BRANIN_HI)
    assert acq.compute(x[None, :])[0] >= acq.compute(Xc).max() - 1e-9
    x = DeviceGradientAscent(acq, BRANIN_LO, BRANIN_HI, n_samples=300, n_starts=4, n_steps=4,
                             rng=np.random.RandomState(5)).maximize()
    assert np.all(x >= BRANIN_LO) and np.all(x <= BRANIN_HI)

    # what has no gradient on the device says so
    class Other(BaseAcquisitionFunction):
        def compute(self, x, derivative=False):
            return np.zeros(len(x))

    class Foreign(object):
        def predict(self, X):
            return np.zeros(len(X)), np.ones(len(X))

        def get_incumbent(self):
            return np.zeros(2), 0.0
    from robo_amd.acquisition_functions import InformationGain, InformationGainMC
    assert InformationGain.refine is BaseAcquisitionFunction.refine and InformationGainMC.refine is BaseAcquisitionFunction.refine
    for bad in (lambda: Other(m).refine(Xc), lambda: EI(Foreign()).refine(Xc),
                lambda: LCB(model(0.3, normalize_input=False)).refine(Xc),
                lambda: MarginalizationGPMCMC(Other(mix)).refine(Xc),
                lambda: DeviceGradientAscent(Other(m), BRANIN_LO, BRANIN_HI).maximize(),
                lambda: DeviceGradientAscent(EI(Foreign()), BRANIN_LO, BRANIN_HI).maximize()):
        with pytest.raises(TypeError):
            bad()


def test_classes(emu_ctx):
    _check_classes(emu_ctx)


def _check_front_end():
    from robo_amd.fmin import bayesian_optimization
    runs = [bayesian_optimization(_branin, BRANIN_LO, BRANIN_HI, num_iterations=6, maximizer="device_gradient",
                                  model_type="gp", n_candidates=2000, rng=np.random.RandomState(7)) for _ in range(2)]
    r = runs[0]
    assert len(r["X"]) == 6
    assert all(np.all(BRANIN_LO <= np.asarray(x)) and np.all(np.asarray(x) <= BRANIN_HI) for x in r["X"])
    assert np.all(np.diff(r["incumbent_values"]) <= 0)
    assert runs[0]["X"] == runs[1]["X"] and runs[0]["y"] == runs[1]["y"]
    with pytest.raises(ValueError):
        bayesian_optimization(_branin, BRANIN_LO, BRANIN_HI, maximizer="gradient")


def test_front_end(emu_ctx):
    _check_front_end()


@pytest.mark.gpu
def test_front_end_gpu(gpu_ctx):
    _check_classes(gpu_ctx)
    _check_front_end()
    from robo_amd.fmin import bayesian_optimization
    r = bayesian_optimization(_branin, BRANIN_LO, BRANIN_HI, num_iterations=5, maximizer="device_gradient",
                              model_type="gp_mcmc", acquisition_func="log_ei", n_candidates=4096, chain_length=20,
                              burnin_steps=20, rng=np.random.RandomState(2))
    assert len(r["X"]) == 5 and np.all(np.diff(r["incumbent_values"]) <= 0)
