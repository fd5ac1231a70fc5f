"""Gradient refinement of the constrained-EI maximum (robo_amd/csrc/cei_refine.hip, api_cei.hip: robo_cei_refine_cand;
ConstrainedEI.refine / value_and_gradient, DeviceGradientAscent, constrained_optimization(maximizer="device_gradient"))
against tests/cei_refine_oracle.py.

As in tests/test_refine.py whole trajectories are not compared: every entry of the device's trace is checked on its own --
value and gradient against the oracle at the device's own trial point, the decisions (accept bit, step length, trial point,
codes) against the rule applied to the device's own stored doubles, bit for bit.

The value's bound is derived in tests/cei_refine_oracle.py (the conditioning of log Phi fed with the posterior tolerances of
tests/_tol.py, plus cei_oracle's bound of the fold); the gradient's is test_refine.py's G_RTOL |g| + G_ATOL_REL max|g|.
Neither is tuned.  Largest observed (value error / bound, gradient error / its bound) are printed per case and recorded in
NOTES.md "Refining the constrained pick".

CPU: through the interpreter (tests/hipemu).  -m gpu: the same checks at the same shapes on the MI355X, plus one case past
the toy size (N = 1100 / 700 / 300, D = 16, C = 2, 8192 candidates, 64 starts, 20 steps).
"""
import os
import sys

import numpy as np
import pytest

from robo_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import cei_oracle as CO  # noqa: E402
import cei_refine_oracle as CRO  # noqa: E402
import refine_oracle as RO  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402

G_RTOL, G_ATOL_REL = 1e-7, 1e-8        # tests/test_refine.py's figures for the gradient
PAR = 0.01
SMALL = dict(D=3, M=400, K=6, T=8, Ns=(80, 130, 257))
MANY = dict(SMALL, M=32, K=4, T=2)      # C = 16: 17 solves per trial, fewer candidates and trials
LARGE = dict(D=16, M=8192, K=64, T=20, Ns=(1100, 700, 300))


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


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- models ------------------------------------------------------------------------------------------------------------------
def _theta(D, ls2, noise=1e-2, amp=0.0):
    return np.concatenate([[amp], np.log(np.broadcast_to(ls2, (D,))), [np.log(noise)]])


def _pair(ctx, kind, theta, X, y, transform=(0.0, 1.0)):
    """the same GP as an oracle model (OracleGP, y_mean, y_std) and on the device (inputs already in [0, 1]^D)"""
    ogp = O.OracleGP(kind, theta, normalize_input=False)
    ogp.train(X, y)
    g = _lib.DeviceGP(ctx, kind, X.shape[0], X.shape[1])
    g.set_data(X, y)
    if transform != (0.0, 1.0):
        g.set_output_transform(*transform)
    g.fit(theta, ogp.mean)
    return (ogp, transform[0], transform[1]), g


class _Setup(object):
    """objective: Matern-5/2 on Ns[0] points; constraint 1: RBF on Ns[1] points with an output transform; constraint 2:
    Matern-5/2 on Ns[2] points with other length scales.  The thresholds are the medians of the constraints' posterior means
    over the candidates, so the feasible region's boundary runs through the box.  constraints(C) cycles through
    (constraint 1, constraint 2, the objective's GP) with thresholds shifted per round: C = 16 from three fits."""

    def __init__(self, ctx, sz, seed=0):
        D, Ns = sz["D"], sz["Ns"]
        rs = np.random.RandomState(seed)
        X = rs.rand(max(Ns), D)
        w = np.sqrt(D / 3.0)
        y = np.sin(3 * X.sum(axis=1) / w) + 0.1 * rs.randn(len(X))
        c1 = np.cos(2 * X[:, 0] - X[:, -1] + 0.3) + 0.5 * (X[:, D // 2] - 0.3) ** 2 + 0.05 * rs.randn(len(X))
        c2 = (X ** 2).sum(axis=1) / D - X[:, 0] * 0.4 + 0.05 * rs.randn(len(X))
        ls = np.array([0.3, 0.5, 0.8, 0.4, 0.6])[:D] if D <= 5 else np.full(D, 0.25 * D)
        self.ctx, self.sz, self.rs, self.y = ctx, sz, rs, y[:Ns[0]]
        self.models, self.gps = [], []
        for kind, theta, n, t, tr in (("matern52", _theta(D, ls), Ns[0], y, (0.0, 1.0)),
                                      ("rbf", _theta(D, ls * 1.7, noise=3e-2, amp=0.3), Ns[1], c1, (0.7, 2.5)),
                                      ("matern52", _theta(D, ls * 0.8, noise=2e-2), Ns[2], c2, (0.0, 1.0))):
            m, g = _pair(ctx, kind, theta, X[:n], t[:n], tr)
            self.models.append(m)
            self.gps.append(g)
        self.Xc = rs.rand(sz["M"], D)
        self.eta = float(np.sort(self.y)[len(self.y) // 4])
        self.th3 = [float(np.median(CRO.model_moments(m, self.Xc[:200])[0])) for m in self.models[1:] + self.models[:1]]
        self.cand = _lib.Candidates(ctx, self.Xc)

    def constraints(self, C):
        order = [1, 2, 0]
        idx = [order[k % 3] for k in range(C)]
        th = np.array([self.th3[k % 3] + 0.15 * (k // 3) for k in range(C)])
        return [self.models[i] for i in idx], [self.gps[i] for i in idx], th

    def close(self):
        self.cand.close()
        for g in self.gps:
            g.close()


# ---- the trace replay (tests/test_refine.py's, restated) ------------------------------------------------------------------------
def _replay(trace, starts, step0, floored=None):
    """every (t, k) of a trace against the rule, on the device's own doubles -> (f at the start, final f, final x);
    floored(y) -> bool, if given: does some solved GP's oracle variance sit on its floor at y (code 3 marks it)"""
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
        alpha, frozen = step0, trace[0, k, -1] == 3
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
            if code == 3 or not np.isfinite(fy):
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


def _result_checks(r, f0, fT, xT):
    used = r.starts >= 0
    assert np.all(fT[used] >= f0[used])
    best = int(np.argmax(np.where(used, fT, -np.inf)))
    assert r.value == fT[best] and r.start_index == r.starts[best]
    np.testing.assert_array_equal(r.x, xT[best])


def _against_oracle(trace, starts, models, th, kind, eta, label):
    """value and gradient of every trace entry against the oracle at the device's own trial point (entries with a floored
    variance excepted: there the posterior tolerances say nothing) -> (largest value error / bound, gradient error / bound)"""
    D = (trace.shape[2] - 3) // 2
    used = starts >= 0
    P = trace[:, used, :D].reshape(-1, D)
    fd = trace[:, used, D].ravel()
    gd = trace[:, used, D + 1:2 * D + 1].reshape(-1, D)
    orc = CRO.evaluate(models, th, kind, PAR, eta, P)
    ok = ~orc["floored"]
    rv = CO.check(fd[ok], dict(value=orc["value"][ok], bound=orc["bound"][ok]))
    go = orc["grad"][ok]
    gmax = np.abs(go).max()
    gb = G_RTOL * np.abs(go) + G_ATOL_REL * gmax
    with np.errstate(invalid="ignore", divide="ignore"):
        rg = float(np.nanmax(np.where(gb > 0, np.abs(gd[ok] - go) / gb, 0.0))) if gmax > 0 else float(np.abs(gd[ok]).max() > 0)
    z = orc["z"]
    print("%s %s eta %s: %d points, z in [%.1f, %.1f], value error / bound %.3g, gradient error / bound %.3g"
          % (label, kind, eta, ok.sum(), z.min() if z.size else 0.0, z.max() if z.size else 0.0, rv, rg))
    assert rv <= 1.0 and rg <= 1.0, (label, kind, eta, rv, rg)
    assert np.all(np.isfinite(gd[ok]) | ~np.isfinite(fd[ok])[:, None])
    return rv, rg


# ---- 0. the oracle's gradient (pure CPU) --------------------------------------------------------------------------------------
def test_oracle_gradient_against_central_differences():
    rs = np.random.RandomState(5)
    X = rs.rand(70, 3)
    y = np.sin(3 * X.sum(axis=1)) + 0.1 * rs.randn(70)
    models = []
    for kind, ls, tr, t in (("matern52", [0.3, 0.5, 0.8], (0.0, 1.0), y), ("rbf", [0.6, 0.4, 0.9], (0.7, 2.5), np.cos(2 * X[:, 0] - X[:, 2])),
                            ("matern52", [0.5, 0.5, 0.5], (0.0, 1.0), (X ** 2).sum(axis=1))):
        ogp = O.OracleGP(kind, _theta(3, ls), normalize_input=False)
        ogp.train(X, t)
        models.append((ogp, tr[0], tr[1]))
    P = 0.05 + 0.9 * rs.rand(30, 3)
    h = 1e-5
    seen = []
    for shift in (-6.0, -2.0, 0.0, 2.0):
        m1, v1 = CRO.model_moments(models[1], P)[:2]
        m2, v2 = CRO.model_moments(models[2], P)[:2]
        th = [float(np.median(m1 + shift * np.sqrt(v1))), float(np.median(m2 - shift * np.sqrt(v2)))]
        for kind in ("ei", "log_ei"):
            for eta in (float(y.min() + 0.3), None):
                fn = CRO.evaluator(models, th, kind, PAR, eta)
                f, g = fn(P)
                seen.append(CRO.evaluate(models, th, kind, PAR, eta, P)["z"].ravel())
                for d in range(3):
                    e = np.zeros(3)
                    e[d] = h
                    num = (fn(P + e)[0] - fn(P - e)[0]) / (2 * h)
                    np.testing.assert_allclose(g[:, d], num, rtol=2e-5, atol=1e-6 * max(1e-300, np.abs(g).max()))
    seen = np.concatenate(seen)
    assert seen.min() < -6.0 and seen.max() > 6.0
    # phi / Phi: the device's fp64 form against the extended-precision one, -40 .. 40, across the switch at -1
    z = np.concatenate((np.linspace(-40.0, 40.0, 801), [-1.0, np.nextafter(-1.0, -2.0)]))
    ref = np.asarray(CO.norm_cdf_pair(z)[2], dtype=np.float64)
    got = CRO.ratio64(z)
    err = np.abs(got - ref) / np.maximum(ref, 1e-300)
    print("phi / Phi in fp64 against np.longdouble: max relative error %.2e" % err[ref > 1e-300].max())
    # left: erfcx's few units; right: exp(-z^2 / 2) answers the rounding of its argument by z^2 / 2 units
    keep = ref > 1e-290
    assert np.all(err[keep] <= (np.where(z > 0, z * z, 0.0)[keep] + 16) * np.finfo(float).eps) and np.all(np.isfinite(got))


# ---- 1. - 3. every entry, every decision, the identities ---------------------------------------------------------------------
def _refine(s, C, kind, eta, K=None, T=None, diagnostics=True, cand=None):
    models, gps, th = s.constraints(C)
    K, T = s.sz["K"] if K is None else K, s.sz["T"] if T is None else T
    r = s.gps[0].cei_refine(gps, cand or s.cand, th, kind, PAR, eta, K, T, 0.05, diagnostics=diagnostics)
    return r, [s.models[0]] + models, gps, th


def _check_steps(ctx, sz, cases, label, seed=0):
    s = _Setup(ctx, sz, seed)
    K, T, D = sz["K"], sz["T"], sz["D"]
    worst = [0.0, 0.0]
    try:
        for C, kind, has_eta in cases:
            eta = s.eta if has_eta else None
            tag = "%s C = %d" % (label, C)
            sweep = s.gps[0].cei(s.constraints(C)[1], s.cand, s.constraints(C)[2], kind, PAR, eta)
            r, models, gps, th = _refine(s, C, kind, eta)
            assert r.trace.shape == (T + 1, K, 2 * D + 3) and np.all(r.starts >= 0), tag
            # the starts: the K best of the fused call's own values
            np.testing.assert_array_equal(r.starts, RO.select(sweep.values, K))
            np.testing.assert_array_equal(r.trace[0, :, :D], s.Xc[r.starts])
            f0, fT, xT = _replay(r.trace, r.starts, 0.05)
            _result_checks(r, f0, fT, xT)
            rv, rg = _against_oracle(r.trace, r.starts, models, th, kind, eta, tag)
            worst = [max(worst[0], rv), max(worst[1], rg)]
            # without diagnostics: the same answer; n_steps = 0: the sweep's own argmax, point and value
            r2, _, _, _ = _refine(s, C, kind, eta, diagnostics=False)
            assert r2.value == r.value and r2.start_index == r.start_index and _bits(r2.x, r.x) and r2.flags == r.flags
            r0, _, _, _ = _refine(s, C, kind, eta, T=0, diagnostics=False)
            assert _bits([r0.value], [sweep.max]) and r0.start_index == sweep.argmax and _bits(r0.x, s.Xc[sweep.argmax]), tag
            # a start's trajectory does not depend on K or on its slot
            rk, _, _, _ = _refine(s, C, kind, eta, K=3)
            np.testing.assert_array_equal(rk.trace, r.trace[:, :3])
            if C == 0 and has_eta:        # robo_acq_refine_cand's result and trace, bit for bit
                p = s.gps[0].refine(kind, PAR, eta, s.cand, K, T, 0.05, diagnostics=True)
                assert _bits(p.trace, r.trace) and _bits(p.x, r.x) and _bits([p.value], [r.value]), tag
                np.testing.assert_array_equal(p.starts, r.starts)
                assert (p.start_index, p.flags) == (r.start_index, r.flags)
    finally:
        s.close()
    print("%s: largest value error / bound %.3g, gradient error / bound %.3g" % (label, worst[0], worst[1]))


SMALL_CASES = [(C, kind, 1) for C in (0, 1, 2) for kind in ("ei", "log_ei")] + [(1, "ei", 0), (2, "log_ei", 0)]


@pytest.mark.parametrize("case", SMALL_CASES, ids=lambda c: "C%d-%s-eta%d" % c)
def test_every_step(emu_ctx, case):
    _check_steps(emu_ctx, SMALL, [case], "interpreter")


@pytest.mark.parametrize("kind", ["log_ei", "ei"])
def test_every_step_16_constraints(emu_ctx, kind):
    _check_steps(emu_ctx, MANY, [(16, kind, 1)], "interpreter")


@pytest.mark.parametrize("D", [1, 17])
def test_every_step_other_dimensions(emu_ctx, D):
    _check_steps(emu_ctx, dict(SMALL, D=D, M=150, K=4, T=4), [(2, "log_ei", 1)], "interpreter D = %d" % D)


def test_every_step_one_start(emu_ctx):
    _check_steps_k1(emu_ctx)


def _check_steps_k1(ctx):
    s = _Setup(ctx, dict(SMALL, M=150))
    try:
        r, models, gps, th = _refine(s, 2, "log_ei", s.eta, K=1)
        f0, fT, xT = _replay(r.trace, r.starts, 0.05)
        _result_checks(r, f0, fT, xT)
        _against_oracle(r.trace, r.starts, models, th, "log_ei", s.eta, "K = 1")
        r6, _, _, _ = _refine(s, 2, "log_ei", s.eta, K=6)
        np.testing.assert_array_equal(r.trace, r6.trace[:, :1])
    finally:
        s.close()


@pytest.mark.gpu
def test_every_step_gpu(gpu_ctx):
    _check_steps(gpu_ctx, SMALL, SMALL_CASES, "MI355X")
    _check_steps(gpu_ctx, MANY, [(16, "log_ei", 1), (16, "ei", 1)], "MI355X")
    for D in (1, 17):
        _check_steps(gpu_ctx, dict(SMALL, D=D, M=150, K=4, T=4), [(2, "log_ei", 1)], "MI355X D = %d" % D)
    _check_steps_k1(gpu_ctx)


@pytest.mark.gpu
def test_every_step_past_the_toy_size_gpu(gpu_ctx):
    _check_steps(gpu_ctx, LARGE, [(2, "log_ei", 1), (2, "ei", 1)], "MI355X large")


def _check_explicit_inverse(ctx):
    """winv_min_blocks = 2 sends the constraints' factors (two and three block rows) through W = L^-1 and leaves the
    objective's (one block row) on the substitution: the constrained traces change their roundings and nothing else, the
    unconstrained one keeps its bits -- the path is decided per GP"""
    sz = dict(SMALL, M=200, K=5, T=4)

    def traces():
        s = _Setup(ctx, sz)
        try:
            return [_refine(s, C, "log_ei", s.eta)[0].trace for C in (0, 2)]
        finally:
            s.close()
    plain = traces()
    ctx.set_tuning("winv_min_blocks", 2)
    try:
        _check_steps(ctx, sz, [(2, "log_ei", 1)], "through W")
        through_w = traces()
    finally:
        ctx.set_tuning("winv_min_blocks", None)
    assert _bits(plain[0], through_w[0])
    assert not _bits(plain[1][0], through_w[1][0])
    np.testing.assert_allclose(plain[1][0, :, :-2], through_w[1][0, :, :-2], rtol=1e-9, atol=1e-12)


def test_every_step_through_the_explicit_inverse(emu_ctx):
    _check_explicit_inverse(emu_ctx)


@pytest.mark.gpu
def test_every_step_through_the_explicit_inverse_gpu(gpu_ctx):
    _check_explicit_inverse(gpu_ctx)


def _check_handles(ctx):
    """EI's sweep on the same handles before and after: the same bits; a later constrained call on used handles equals the
    call on fresh ones; mixed with robo_acq_refine_cand on the objective's GP, whose state block it shares"""
    a, b = _Setup(ctx, dict(SMALL, M=150)), _Setup(ctx, dict(SMALL, M=150))
    try:
        before = a.gps[0].acq("ei", PAR, a.eta, a.cand)
        plain_before = a.gps[0].refine("log_ei", PAR, a.eta, a.cand, 4, 3, 0.05, diagnostics=True)
        first, _, _, _ = _refine(a, 2, "log_ei", a.eta)
        _refine(a, 1, "ei", None, K=3)
        _refine(a, 4, "ei", a.eta, K=9, T=1)
        again, _, _, _ = _refine(a, 2, "log_ei", a.eta)
        fresh, _, _, _ = _refine(b, 2, "log_ei", b.eta)
        for p, q in ((first, again), (first, fresh)):
            assert _bits(p.trace, q.trace) and _bits(p.x, q.x) and _bits([p.value], [q.value])
            assert (p.start_index, p.flags) == (q.start_index, q.flags) and np.array_equal(p.starts, q.starts)
        after = a.gps[0].acq("ei", PAR, a.eta, a.cand)
        for p, q in zip(before, after):
            assert _bits([p], [q])
        plain_after = a.gps[0].refine("log_ei", PAR, a.eta, a.cand, 4, 3, 0.05, diagnostics=True)
        assert _bits(plain_before.trace, plain_after.trace)
    finally:
        a.close()
        b.close()


def test_handles(emu_ctx):
    _check_handles(emu_ctx)


@pytest.mark.gpu
def test_handles_gpu(gpu_ctx):
    _check_handles(gpu_ctx)


# ---- 4. edges ---------------------------------------------------------------------------------------------------------------------
def _check_tails(ctx, label):
    """thresholds 40 standard deviations below and above the constraint's mean at the best candidates: z_k from -40 to 40.
    At -40 the log form keeps value and gradient finite and climbs; the product form's value has underflowed to 0: no
    direction, every start freezes at once with the flag"""
    s = _Setup(ctx, dict(SMALL, M=150))
    try:
        m1, v1 = CRO.model_moments(s.models[1], s.Xc)[:2]
        zs = []
        s1 = np.sqrt(v1)
        for off in (-40.0, -20.0, -5.0, 5.0, 40.0):
            # -40 / 40: EVERY candidate at least that far out (the starts are the ones nearest to it); between: the median
            t = m1 + off * s1
            th = np.array([float(t.min() if off == -40.0 else t.max() if off == 40.0 else np.median(t))])
            for kind in ("log_ei", "ei"):
                r = s.gps[0].cei_refine(s.gps[1:2], s.cand, th, kind, PAR, s.eta, 6, 6, 0.05, diagnostics=True)
                _replay(r.trace, r.starts, 0.05)
                _against_oracle(r.trace, r.starts, s.models[:2], th, kind, s.eta, "%s tails, off %g" % (label, off))
                D = 3
                z = CRO.evaluate(s.models[:2], th, kind, PAR, s.eta, r.trace[:, :, :D].reshape(-1, D))["z"].reshape(7, 6)
                zs.append(z.ravel())
                if off == -40.0 and kind == "log_ei":
                    assert z[0].max() <= -40.0 and np.all(np.isfinite(r.trace)) and np.any(r.trace[1:, :, -1] == 1)
                    assert np.all(r.trace[0, :, D] < -700) and r.value > r.trace[0, :, D].max()
                if off == -40.0 and kind == "ei":
                    assert np.all(r.trace[:, :, D] == 0.0) and np.all(r.trace[:, :, D + 1:2 * D + 1] == 0.0)
                    assert np.all(r.trace[0, :, -1] == 1) and np.all(r.trace[1:, :, -1] == 2)
                    assert r.flags & _lib.FLAG_FROZEN and r.value == 0.0
                if off == 40.0:
                    assert np.all(np.isfinite(r.trace)) and z[0].min() >= 40.0
        z = np.concatenate(zs)
        assert z.min() < -38.0 and z.max() > 38.0
    finally:
        s.close()


def test_tails(emu_ctx):
    _check_tails(emu_ctx, "interpreter")


@pytest.mark.gpu
def test_tails_gpu(gpu_ctx):
    _check_tails(gpu_ctx, "MI355X")


def _check_edges(ctx):
    rs = np.random.RandomState(3)
    X = rs.rand(60, 2)
    y = np.sin(3 * X.sum(axis=1)) + 0.1 * rs.randn(60)
    c = 1.2 - X[:, 0] - X[:, 1] + 0.02 * rs.randn(60)                 # feasible towards the corner (1, 1)
    mo, go = _pair(ctx, "matern52", _theta(2, [0.3, 0.5]), X, y)
    mc, gc = _pair(ctx, "rbf", _theta(2, [0.8, 0.8], noise=1e-3), X, c)
    # a constraint whose variance at its training points sits below the floor (output scale 1e-4, noise 1e-8)
    mf, gf = _pair(ctx, "matern52", _theta(2, [0.3, 0.5], noise=1e-8), X, c, transform=(0.0, 1e-4))
    handles = [go, gc, gf]
    try:
        # starts on a face and in a corner: the trial points stay in the box, the replay's projection holds bit for bit
        Xc = rs.rand(200, 2)
        Xc[:60, 1] = 1.0
        Xc[0], Xc[1] = [1.0, 1.0], [0.0, 1.0]
        cand = _lib.Candidates(ctx, Xc)
        handles.append(cand)
        for kind in ("log_ei", "ei"):
            r = go.cei_refine([gc], cand, [0.0], kind, PAR, float(y.min()), 8, 8, 0.05, diagnostics=True)
            f0, fT, xT = _replay(r.trace, r.starts, 0.05)
            _result_checks(r, f0, fT, xT)
            _against_oracle(r.trace, r.starts, [mo, mc], [0.0], kind, float(y.min()), "face")
            on_face = r.trace[0, :, 1] == 1.0
            assert on_face.sum() >= 3
        pin = _lib.Candidates(ctx, np.array([[1.0, 1.0], [0.0, 1.0], [1.0, 0.0], [0.0, 0.0], [1.0, 0.5]]))
        handles.append(pin)
        r = go.cei_refine([gc], pin, [0.0], "log_ei", PAR, float(y.min()), 5, 6, 0.05, diagnostics=True)
        _replay(r.trace, r.starts, 0.05)
        assert sorted(r.starts.tolist()) == [0, 1, 2, 3, 4] and np.all((r.trace[:, :, :2] >= 0) & (r.trace[:, :, :2] <= 1))
        # the floor in a CONSTRAINT's GP only: code 3 at once for starts on its training points, and for trials landing there
        def floored(p):
            return bool(CRO.model_moments(mf, np.atleast_2d(p))[4][0])
        Xf = np.vstack([X[:4], rs.rand(8, 2), X[4:9] + 1e-3])
        assert all(floored(p) for p in Xf[:4]) and not any(floored(p) for p in Xf[4:12])
        assert not CRO.model_moments(mo, Xf)[4].any()
        cf = _lib.Candidates(ctx, Xf)
        handles.append(cf)
        for kind, eta in (("log_ei", float(y.min())), ("ei", None)):
            r = go.cei_refine([gf], cf, [0.0], kind, PAR, eta, len(Xf), 10, 0.05, diagnostics=True)
            _replay(r.trace, r.starts, 0.05, floored)
            on_data = np.isin(r.starts, np.arange(4))
            assert on_data.sum() == 4 and np.all(r.trace[0, on_data, -1] == 3) and np.all(r.trace[1:, on_data, -1] == 2)
            np.testing.assert_array_equal(r.trace[0, :, -1], np.where([floored(p) for p in Xf[r.starts]], 3, 1))
            assert r.flags & _lib.FLAG_FROZEN
        # a NaN candidate is never a start; fewer eligible candidates than starts
        Xn = rs.rand(12, 2)
        Xn[[0, 2, 3, 5, 8, 9, 11], 0] = np.nan
        cn = _lib.Candidates(ctx, Xn)
        handles.append(cn)
        vals = go.cei([gc], cn, [0.0], "log_ei", PAR, float(y.min())).values
        for K2 in (3, 8):
            r = go.cei_refine([gc], cn, [0.0], "log_ei", PAR, float(y.min()), K2, 2, 0.05, diagnostics=True)
            want = np.full(K2, -1)
            order = RO.select(vals, K2)
            want[:len(order)] = order
            np.testing.assert_array_equal(r.starts, want)
            _replay(r.trace, r.starts, 0.05)
            assert r.flags & _lib.FLAG_NAN and np.isfinite(r.value) and np.all(np.isfinite(r.x)) and r.start_index in order
    finally:
        for h in handles:
            h.close()


def test_edges(emu_ctx):
    _check_edges(emu_ctx)


@pytest.mark.gpu
def test_edges_gpu(gpu_ctx):
    _check_edges(gpu_ctx)


def _check_no_incumbent_skips_the_objective(ctx):
    """has_eta = 0: the iterations never solve the objective's GP.  Its factor (three block rows) does not fit a workspace
    that holds the 128 pseudo-rows of the constraint's (one block row): with an incumbent the call is refused, without one
    it runs, in both forms, and its values are the oracle's PoF / L of the constraint alone"""
    s = _Setup(ctx, dict(SMALL, M=150, Ns=(257, 80, 80)))
    try:
        th = np.array([s.th3[0]])
        ctx.set_tuning("ws_bytes", 128 * 128 * 8)
        try:
            with pytest.raises(_lib.RoboBadShape):
                s.gps[0].cei_refine(s.gps[1:2], s.cand, th, "log_ei", PAR, s.eta, 6, 4, 0.05)
            got = {kind: s.gps[0].cei_refine(s.gps[1:2], s.cand, th, kind, PAR, None, 6, 4, 0.05, diagnostics=True)
                   for kind in ("ei", "log_ei")}
        finally:
            ctx.set_tuning("ws_bytes", None)
        for kind, r in got.items():
            _replay(r.trace, r.starts, 0.05)
            _against_oracle(r.trace, r.starts, s.models[:2], th, kind, None, "no incumbent")
            full = s.gps[0].cei_refine(s.gps[1:2], s.cand, th, kind, PAR, None, 6, 4, 0.05, diagnostics=True)
            assert _bits(full.trace, r.trace)
        # with no constraint either the value is constant: every start is evaluated, has no direction and freezes
        r = s.gps[0].cei_refine([], s.cand, [], "ei", PAR, None, 4, 3, 0.05, diagnostics=True)
        assert np.all(r.trace[:, :, 3] == 1.0) and np.all(r.trace[1:, :, -1] == 2) and r.value == 1.0
        np.testing.assert_array_equal(r.starts, np.arange(4))
    finally:
        s.close()


def test_no_incumbent_skips_the_objective(emu_ctx):
    _check_no_incumbent_skips_the_objective(emu_ctx)


@pytest.mark.gpu
def test_no_incumbent_skips_the_objective_gpu(gpu_ctx):
    _check_no_incumbent_skips_the_objective(gpu_ctx)


def test_refusals(emu_ctx):
    ctx = emu_ctx
    s = _Setup(ctx, dict(SMALL, M=64))
    rs = s.rs
    other = _lib.Context(0)
    g0, cons, th = s.gps[0], s.gps[1:], np.array(s.th3[:2])
    eta = s.eta
    wide = _lib.Candidates(ctx, rs.rand(5, 4))
    far = _lib.Candidates(other, s.Xc[:5])
    Xo = rs.rand(20, 3)
    g_far = _lib.DeviceGP(other, "rbf", 20, 3)
    g_far.set_data(Xo, Xo[:, 0])
    g_far.fit(_theta(3, 0.5), 0.5)
    raw = _lib.DeviceGP(ctx, "matern52", 80, 3)
    fab = _lib.DeviceGP(ctx, "fabolas", 20, 3)
    fab.set_data(Xo, Xo[:, 0])
    fab.fit(np.concatenate([[0.0], np.log([0.5, 0.5]), [np.log(0.5), np.log(0.8)], [np.log(1e-2)]]), 0.5)
    try:
        def run(obj=g0, c=cons, cand=s.cand, t=th, kind="ei", par=0.0, e=eta, K=4, T=2, s0=0.05):
            return obj.cei_refine(c, cand, t, kind, par, e, K, T, s0)
        for kw in (dict(K=0), dict(K=1025), dict(T=-1), dict(s0=0.0), dict(s0=0.6), dict(s0=np.nan)):
            with pytest.raises(ValueError):
                run(**kw)
        for kw in (dict(c=[cons[0], g_far]), dict(obj=g_far, c=cons[:1], t=th[:1]), dict(cand=far), dict(c=cons * 9, t=np.tile(th, 9)),
                   dict(t=[th[0], np.nan]), dict(t=[np.inf, th[1]]), dict(e=np.nan), dict(kind="log_ei", par=np.inf),
                   dict(kind="pi"), dict(kind="lcb"), dict(c=[cons[0], fab]), dict(obj=fab, c=[], t=[])):
            with pytest.raises(ValueError):
                run(**kw)
        with pytest.raises(_lib.RoboBadShape):
            run(cand=wide)
        for a, b in ((raw, cons), (g0, [cons[0], raw])):
            with pytest.raises(Exception, match="trained first"):
                run(obj=a, c=b)
        # the workspace must hold the pseudo-rows of the LARGEST factor solved
        ctx.set_tuning("ws_bytes", 128 * 256 * 8)
        try:
            with pytest.raises(_lib.RoboBadShape):
                run()                                     # constraint 2 (257 points) needs more than 256 columns
            assert run(c=cons[:1], t=th[:1]).flags == 0
        finally:
            ctx.set_tuning("ws_bytes", None)
        best, x = _lib._Best(), np.empty(3)
        call = _lib.lib().robo_cei_refine_cand
        hs, tharr = _lib._handles(cons), np.ascontiguousarray(th)
        tail = (4, 2, 0.05, _lib._arr(x)) + best.refs + (None, None)
        mid = (0, 0.0, eta, 1)
        assert call(None, hs, 2, _lib._arr(tharr), *mid, s.cand._h, *tail) == _lib.BAD_ARGUMENT
        assert call(g0._h, None, 2, _lib._arr(tharr), *mid, s.cand._h, *tail) == _lib.BAD_ARGUMENT
        assert call(g0._h, hs, 2, None, *mid, s.cand._h, *tail) == _lib.BAD_ARGUMENT
        assert call(g0._h, hs, 2, _lib._arr(tharr), *mid, None, *tail) == _lib.BAD_ARGUMENT
        assert call(g0._h, hs, -1, _lib._arr(tharr), *mid, s.cand._h, *tail) == _lib.BAD_ARGUMENT
        assert call(g0._h, hs, 2, _lib._arr(tharr), *mid, s.cand._h, 4, 2, 0.05, None, *best.refs, None, None) == _lib.BAD_ARGUMENT
        ok = run()                                        # the handles are still usable, no stale flags
        assert ok.flags == 0 and np.isfinite(ok.value)
    finally:
        for h in (wide, far, g_far, raw, fab):
            h.close()
        other.close()
        s.close()


# ---- 5. it does what it is for --------------------------------------------------------------------------------------------------
def _check_active_constraint(ctx, label):
    """D = 2: the objective falls towards (0.2, 0.2), the constraint x_0 + x_1 >= 0.9 cuts that corner off, so the constrained
    optimum sits on the boundary, which 300 random candidates only straddle.  8 starts, 60 steps."""
    rs = np.random.RandomState(8)
    X = rs.rand(40, 2)
    y = ((X - 0.2) ** 2).sum(axis=1) + 0.01 * rs.randn(40)
    c = 0.9 - X[:, 0] - X[:, 1] + 0.01 * rs.randn(40)
    mo, go = _pair(ctx, "matern52", _theta(2, [0.6, 0.6], noise=1e-3), X, y)
    mc, gc = _pair(ctx, "matern52", _theta(2, [0.9, 0.9], noise=1e-3), X, c)
    Xc = rs.rand(300, 2)
    cand = _lib.Candidates(ctx, Xc)
    feas = c <= 0.0
    eta = float(y[feas].min())
    g1 = np.linspace(0.0, 1.0, 129)
    G = np.array(np.meshgrid(g1, g1)).reshape(2, -1).T
    try:
        for kind in ("log_ei", "ei"):
            sweep = go.cei([gc], cand, [0.0], kind, PAR, eta)
            r = go.cei_refine([gc], cand, [0.0], kind, PAR, eta, 8, 60, 0.05)
            grid = np.asarray(CRO.evaluate([mo, mc], [0.0], kind, PAR, eta, G)["value"], dtype=np.float64)
            p_ref, p_sweep = CRO.pof([mo, mc], [0.0], np.vstack([r.x, Xc[sweep.argmax]]))
            print("%s %s: sweep %.12g, grid %.12g, refined %.12g at %s; PoF %.6f (sweep pick %.6f)"
                  % (label, kind, sweep.max, grid.max(), r.value, r.x, p_ref, p_sweep))
            assert r.value >= sweep.max and r.value >= grid.max()
            assert p_ref >= p_sweep
    finally:
        for h in (cand, go, gc):
            h.close()


def test_active_constraint(emu_ctx):
    _check_active_constraint(emu_ctx, "interpreter")


@pytest.mark.gpu
def test_active_constraint_gpu(gpu_ctx):
    _check_active_constraint(gpu_ctx, "MI355X")


# ---- 6. classes and front end ----------------------------------------------------------------------------------------------------
_BOX = (np.array([-1.0, 0.0]), np.array([1.0, 2.0]))
_TH2 = np.array([0.0, 0.15])


def _toy2(x):
    u = (np.asarray(x, dtype=np.float64) - _BOX[0]) / (_BOX[1] - _BOX[0])
    return float(np.sum((u - 0.2) ** 2)), float(0.9 - u[0] - u[1]), float(u[0] - 0.6)


def _gp_models(n=14, seed=0):
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models import GaussianProcess
    rs = np.random.RandomState(seed)
    X = _BOX[0] + (_BOX[1] - _BOX[0]) * rs.rand(n, 2)
    Y = np.array([_toy2(x) for x in X])
    models = []
    for o, ls in enumerate((0.6, 0.9, 0.7)):
        m = GaussianProcess(Matern52Kernel(np.array([ls, ls]), ndim=2), noise=1e-3, lower=_BOX[0], upper=_BOX[1],
                            normalize_output=bool(o == 1))
        m.train(X, Y[:, o].copy(), do_optimize=False)
        models.append(m)
    return rs, X, Y, models


def _check_classes(ctx):
    from robo_amd.acquisition_functions import ConstrainedEI, EHVI
    from robo_amd.maximizers import DeviceGradientAscent
    rs, X, Y, models = _gp_models()
    Xc = _BOX[0] + (_BOX[1] - _BOX[0]) * rs.rand(120, 2)
    span = _BOX[1] - _BOX[0]
    for log in (False, True):
        acq = ConstrainedEI(models, _TH2, par=PAR, log=log)
        assert acq.eta is not None
        vals = acq.compute(Xc)
        best = Xc[acq.argmax(Xc)]
        x0 = acq.refine(Xc, n_starts=4, n_steps=0)
        np.testing.assert_allclose(x0, best, rtol=0, atol=1e-15)
        assert acq.last_refine.start_index == acq.last_argmax and _bits([acq.last_refine.value], [vals.max()])
        x = acq.refine(Xc, n_starts=6, n_steps=12)
        assert x.shape == (2,) and np.all(x >= _BOX[0]) and np.all(x <= _BOX[1])
        assert acq.last_refine.value >= vals.max() and acq.last_max == acq.last_refine.value
        assert abs(acq.compute(x[None, :])[0] - acq.last_refine.value) <= 1e-7 * abs(acq.last_refine.value)
        rd = acq.refine(Xc, n_starts=6, n_steps=12, diagnostics=True)
        np.testing.assert_array_equal(rd, x)
        assert acq.last_refine.trace.shape == (13, 6, 7)
        # value_and_gradient: the sweep's values to rounding, the gradient against central differences of compute()
        P = _BOX[0] + span * (0.1 + 0.8 * rs.rand(9, 2))
        v, g = acq.value_and_gradient(P)
        assert v.shape == (9,) and g.shape == (9, 2)
        np.testing.assert_allclose(v, acq.compute(P), rtol=1e-7, atol=0)
        h = 1e-5
        for d in range(2):
            e = np.zeros(2)
            e[d] = h * span[d]
            num = (acq.compute(P + e) - acq.compute(P - e)) / (2 * h * span[d])
            np.testing.assert_allclose(g[:, d], num, rtol=1e-4, atol=1e-6 * np.abs(g).max())
        # a device batch in the normalised box is the same call
        cand = _lib.Candidates(models[0].gp.ctx, models[0]._normalised(Xc))
        try:
            np.testing.assert_array_equal(acq.refine(cand, n_starts=6, n_steps=12), x)
        finally:
            cand.close()
        with pytest.raises(ValueError):
            acq.value_and_gradient(np.zeros((1025, 2)))
        with pytest.raises(NotImplementedError):
            acq.compute(Xc, derivative=True)
    # no feasible observation: the PoF-only rule is what climbs
    hard = ConstrainedEI(models, [-1.5, -1.0], log=True)
    assert hard.eta is None
    x = hard.refine(Xc, n_starts=4, n_steps=6)
    best = hard.compute(Xc).max()                      # (log form without an incumbent: log PoF itself)
    assert np.isfinite(best) and hard.last_refine.value > best and hard.compute(x[None, :])[0] >= best
    # the maximiser draws around the feasible incumbent and refines
    acq = ConstrainedEI(models, _TH2, log=True)
    x = DeviceGradientAscent(acq, _BOX[0], _BOX[1], n_samples=256, n_starts=4, n_steps=6, rng=np.random.RandomState(5)).maximize()
    assert x.shape == (2,) and np.all(x >= _BOX[0]) and np.all(x <= _BOX[1])
    again = DeviceGradientAscent(acq, _BOX[0], _BOX[1], n_samples=256, n_starts=4, n_steps=6, rng=np.random.RandomState(5)).maximize()
    np.testing.assert_array_equal(x, again)
    # refusals

    class Foreign(object):
        def __init__(self, m):
            self._m, self.X, self.y, self.lower, self.upper = m, m.X, m.y, m.lower, m.upper
            self.normalize_input = True

        def predict(self, Xq):
            return self._m.predict(Xq)
    foreign = ConstrainedEI([models[0], Foreign(models[1]), models[2]], _TH2)
    for call in (lambda: foreign.refine(Xc), lambda: foreign.value_and_gradient(Xc[:3]),
                 lambda: DeviceGradientAscent(EHVI(models[:2], [5.0, 5.0]), _BOX[0], _BOX[1]).maximize()):
        with pytest.raises(TypeError):
            call()
    models[2].devices = [0, 1]
    try:
        with pytest.raises(NotImplementedError, match="devices"):
            acq.refine(Xc)
    finally:
        models[2].devices = None
    from robo_amd.models.fabolas_gp import FabolasGP
    fab = FabolasGP.__new__(FabolasGP)
    with pytest.raises(TypeError, match="Fabolas"):
        ConstrainedEI.refine(_with_models(acq, [models[0], fab, models[2]]), Xc)


def _with_models(acq, models):
    """a shallow stand-in for ``acq`` over other models (no observation is read: refine refuses before)"""
    import copy
    from robo_amd.acquisition_functions.constrained_ei import ConstrainedModels
    dup = copy.copy(acq)
    dup.model = ConstrainedModels(models[0], models[1:], acq.thresholds)
    return dup


def test_classes(emu_ctx):
    _check_classes(emu_ctx)


def _check_front_end(label):
    """3 initial points + 3 iterations, 96 device candidates, 4 starts, 6 steps, seeded.  Every proposal is replayed from
    the maximiser's seed: the candidates are drawn again on the device, the refinement runs again with its trace, and
    the trace's winner must be the proposal; the value the device reports for it must be the oracle-checked sweep's rule
    (ConstrainedEI.compute at the proposal, to ACQ_RTOL) and no lower than the candidates' best."""
    from robo_amd.fmin import constrained_optimization
    FE = sys.modules["robo_amd.fmin.constrained_optimization"]
    from robo_amd.maximizers import DeviceGradientAscent
    seen = []

    class Replayed(DeviceGradientAscent):
        def maximize(self, q=None):
            acq = self.objective_func
            own = self.rng.get_state()
            x = super(Replayed, self).maximize()
            self.rng.set_state(own)
            seed = int(self.rng.randint(0, 2 ** 31 - 1))                       # the draw maximize() made
            obj = acq.model.objective
            lower, upper = np.asarray(obj.lower), np.asarray(obj.upper)
            inc = np.asarray(acq.model.get_incumbent()[0], dtype=np.float64)
            cand = _lib.Candidates(obj.gp.ctx, m=self.n_samples, seed=seed, n_uniform=int(self.n_samples * .7),
                                   loc=(inc - lower) / (upper - lower), scale=0.1 / (upper - lower))
            try:
                sweep = acq.compute(cand)
                r = obj.gp.cei_refine([m.gp for m in acq.model.constraints], cand, acq.thresholds, acq.kind, acq.par, acq.eta,
                                      self.n_starts, self.n_steps, self.step0, diagnostics=True)
                np.testing.assert_array_equal(r.starts, RO.select(sweep, self.n_starts))
                f0, fT, xT = _replay(r.trace, r.starts, self.step0)
                _result_checks(r, f0, fT, xT)
                np.testing.assert_array_equal(lower + (upper - lower) * r.x, x)
                assert r.value >= np.nanmax(sweep)
                at_x = acq.compute(np.asarray(x)[None, :])[0]
                assert abs(at_x - r.value) <= 1e-7 * abs(r.value) + 1e-300, (at_x, r.value)
            finally:
                cand.close()
            seen.append((acq.eta, acq.model.y.shape[0]))
            return x

    FE.DeviceGradientAscent = Replayed
    try:
        for acqf, seed, runs in (("log_cei", 2, 2), ("cei", 1, 1)):
            del seen[:]
            res = [constrained_optimization(_toy2, _BOX[0], _BOX[1], _TH2, num_iterations=6, n_init=3, acquisition_func=acqf,
                                            maximizer="device_gradient", n_candidates=96, rng=np.random.RandomState(seed),
                                            n_starts=4, n_steps=6) for _ in range(runs)]
            assert res[0]["X"] == res[-1]["X"] and len(seen) == 3 * runs
            X = np.array(res[0]["X"])
            assert X.shape == (6, 2) and np.all(X >= _BOX[0]) and np.all(X <= _BOX[1])
            print("%s: constrained_optimization(%s, device_gradient): feasible %s, f_opt %s"
                  % (label, acqf, res[0]["feasible"], res[0]["f_opt"]))
    finally:
        FE.DeviceGradientAscent = DeviceGradientAscent
    from robo_amd.fmin import multi_objective_optimization
    with pytest.raises(ValueError):
        constrained_optimization(_toy2, _BOX[0], _BOX[1], _TH2, maximizer="device_gradient", model_type="gp_mcmc")
    with pytest.raises(ValueError):
        constrained_optimization(_toy2, _BOX[0], _BOX[1], _TH2, maximizer="gradient")
    with pytest.raises(TypeError):
        constrained_optimization(_toy2, _BOX[0], _BOX[1], _TH2, 7, 3, "device_gradient", "gp", "cei", 96, None, "host", 8, 200,
                                 100, 4)                                      # n_starts is keyword-only
    with pytest.raises(ValueError):
        multi_objective_optimization(lambda x: (0.0, 0.0), _BOX[0], _BOX[1], [5.0, 5.0], maximizer="device_gradient")


def test_front_end(emu_ctx):
    _check_front_end("interpreter")


@pytest.mark.gpu
def test_classes_and_front_end_gpu(gpu_ctx):
    _check_classes(gpu_ctx)
    _check_front_end("MI355X")
