"""Refinement of a path's minimiser on the device (robo_amd/csrc/paths_refine.hip, api_paths.hip: robo_paths_descend,
robo_paths_refine_cand; _lib.PosteriorPaths.descend / refine, ThompsonSampling.refine / select_batch(refine=True) /
value_and_gradient, DeviceGradientAscent over a Thompson objective) against tests/paths_grad_oracle.py.

CPU: through the interpreter (tests/hipemu).  -m gpu: the same checks at the same small shapes on the MI355X.

The oracle is the rule of include/robo_hip.h in np.longdouble, fed THE DEVICE'S OWN DOUBLES (scaled rows as cov_oracle.scale
makes them, the same omega, phase, w, eps, and the device's own trial points).  Bounds, per case and path:

    value      |f_dev - f_orc| <= MU_RTOL |f_orc| + MU_ATOL max(1, max |f_orc|) + 20 dev        (tests/test_paths.py's)
    gradient   |g_dev - g_orc| <= 1e-13 max |g_orc| + 20 dev_g                                  (tests/test_v_consumers.py's form)

with dev / dev_g the largest deviation of the same routine in np.float64 from the long-double oracle over the case's points
(they carry the conditioning of alpha).  Largest observed error / bound:
    interpreter:   value 0.037, gradient 0.066 (value cases); 0.025, 0.065 (traces); 0.0005, 0.080 (class replay)
    MI355X:        value 0.072, gradient 0.076 (value cases); 0.024, 0.045 (traces); 0.0005, 0.103 (class replay)
Every decision of a trace (trial point, step length, accept bit, code) is recomputed in NumPy from the device's own stored
doubles and compared bit for bit, so no decision is compared across different arithmetic and no near tie needs excluding.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from robo_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import cov_oracle as CO  # noqa: E402
import paths_grad_oracle as GO  # noqa: E402
import paths_oracle as PO  # noqa: E402
from _tol import MU_ATOL, MU_RTOL  # noqa: E402
from robo_amd.util.spectral import draw_features  # noqa: E402

AMP = 1.3
STEP0 = 0.05
# (kind, N, D, F, S, P, noise, output normalisation): every listed size of every axis, both kinds, both noises
CASES = [
    ("matern52", 1, 1, 1, 1, 1, 1e-2, False),
    ("rbf", 63, 3, 63, 2, 17, 1e-6, True),
    ("matern52", 64, 16, 64, 17, 129, 1e-2, True),
    ("rbf", 65, 17, 65, 64, 17, 1e-2, False),
    ("matern52", 130, 3, 300, 17, 129, 1e-6, False),
    ("rbf", 257, 16, 300, 64, 129, 1e-6, True),
    ("matern52", 257, 17, 1, 2, 1, 1e-2, True),
    ("rbf", 1, 1, 300, 1, 17, 1e-6, False),
    ("matern52", 65, 33, 64, 2, 17, 1e-2, True),                 # the kernel's forms for 33 .. 48 and 49 .. 64 dimensions
    ("rbf", 64, 64, 65, 2, 17, 1e-2, False),
]


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


class _Worst(object):
    value = 0.0
    grad = 0.0


class _Problem(object):
    """one data set, one theta, its draws, P points with their paths (some on box faces, one on a training row)"""

    def __init__(self, kind, N, D, F, S, P, noise, norm, seed=0, target=None):
        rs = np.random.RandomState(1000 * seed + 7 * N + D)
        self.kind, self.N, self.D, self.F, self.S, self.P, self.norm = kind, N, D, F, S, P, norm
        self.X = rs.rand(N, D)
        y = (np.sin(3.0 * self.X.sum(axis=1) / np.sqrt(D)) if target is None else target(self.X)) + 0.1 * rs.randn(N)
        self.y_mean, self.y_std = (float(y.mean()), float(y.std())) if (norm and N > 1) else (0.0, 1.0)
        self.y = (y - self.y_mean) / self.y_std
        self.mean_c = float(self.y.mean())
        self.lnm = np.log(np.linspace(0.3, 0.9, D))
        self.ism = CO.inv_sqrt_metric(self.lnm)
        self.theta = np.concatenate([[np.log(AMP)], self.lnm, [np.log(noise)]])
        self.noise = float(np.exp(self.theta[-1]))
        self.omega, self.phase = draw_features(kind, D, F, rs)
        self.w, self.eps = rs.standard_normal((S, F)), rs.standard_normal((S, N))
        self.x0 = rs.rand(P, D)
        self.x0[0] = self.X[N // 2]                                  # a point equal to a training row
        for i in range(1, P, 3):                                     # points on box faces
            self.x0[i, rs.randint(D)] = float(rs.randint(2))
        self.path_of = rs.randint(S, size=P).astype(np.int32)        # not sorted
        self._orc = {}

    def fit(self, ctx):
        g = _lib.DeviceGP(ctx, self.kind, self.N, self.D)
        g.set_data(self.X, self.y)
        g.set_output_transform(self.y_mean, self.y_std)
        g.fit(self.theta, self.mean_c)
        return g

    def paths(self, g, rows=None):
        rows = slice(None) if rows is None else rows
        return g.sample_paths(self.omega, self.phase, self.w[rows], self.eps[rows])

    def model(self, dtype):
        if dtype not in self._orc:
            self._orc[dtype] = GO.GradPaths(self.kind, AMP, self.noise, CO.scale(self.X, self.lnm), self.y, self.mean_c,
                                            self.omega, self.phase, self.w, self.eps, self.y_mean, self.y_std, dtype=dtype)
        return self._orc[dtype]

    def oracle(self, pts):
        """long-double values (S, m) and gradients (S, m, D) in the unscaled space at normalised points, and the fp64
        model's largest deviation per path: dev (S,), dev_g (S,)"""
        Xs = CO.scale(pts, self.lnm)
        f, g = self.model(PO.LD).values(Xs), self.model(PO.LD).gradients(Xs, self.ism)
        f64, g64 = self.model(np.float64).values(Xs), self.model(np.float64).gradients(Xs, self.ism)
        dev = np.max(np.abs(f64 - f), axis=1).astype(np.float64)
        dev_g = np.max(np.abs(g64 - g), axis=(1, 2)).astype(np.float64)
        return f, g, dev, dev_g


_PROBLEMS = {}


def _problem(*key):
    if key not in _PROBLEMS:
        _PROBLEMS[key] = _Problem(*key)
    return _PROBLEMS[key]


def _check_against_oracle(pr, pts, path_of, val, grad, label, worst):
    """value and gradient of point i on path path_of[i] against the bounds -> the failures"""
    f, g, dev, dev_g = pr.oracle(pts)
    fails = []
    for s in sorted(set(int(v) for v in path_of)):
        at = np.flatnonzero(path_of == s)
        o = np.abs(np.asarray(f[s], dtype=np.float64))
        bound = (MU_RTOL * o + MU_ATOL * max(1.0, float(o.max())) + 20.0 * dev[s])[at]
        err = np.abs(val[at].astype(PO.LD) - f[s][at]).astype(np.float64)
        worst.value = max(worst.value, float(np.max(err / bound)))
        if not np.all(err <= bound):
            fails.append((label, "value", s, float(np.max(err / bound))))
        gb = 1e-13 * float(np.max(np.abs(g[s]))) + 20.0 * dev_g[s]
        gerr = float(np.max(np.abs(grad[at].astype(PO.LD) - g[s][at])))
        worst.grad = max(worst.grad, gerr / gb)
        if not gerr <= gb:
            fails.append((label, "gradient", s, gerr / gb))
    return fails


# ---- 1. the oracle alone (NumPy) ---------------------------------------------------------------------------------------------------
def test_oracle_gradient_is_the_derivative_of_the_oracle_value():
    """the long-double gradient against central differences of the long-double value (h = 1e-6 in the scaled space: the
    truncation error h^2 f''' / 6 and the rounding error eps_ld |f| / h are both below 1e-9 max |g|), both kinds, D = 1 and
    3, including a point that coincides with a training row.  Observed: 2.2e-11 max |g| at the worst."""
    worst = 0.0
    for kind in ("matern52", "rbf"):
        for D in (1, 3):
            rs = np.random.RandomState(40 + D)
            N, F, S = 12, 20, 3
            Xs = rs.rand(N, D) * 1.5
            y = rs.randn(N)
            omega, phase = draw_features(kind, D, F, rs)
            p = GO.GradPaths(kind, AMP, 1e-2, Xs, y, 0.1, omega, phase, rs.standard_normal((S, F)), rs.standard_normal((S, N)),
                             0.3, 1.7)
            pts = rs.rand(6, D) * 1.5
            pts[0] = Xs[4]
            g = p.gradients(pts)
            assert g.shape == (S, 6, D) and g.dtype == PO.LD
            h = PO.LD(1e-6)
            for d in range(D):
                e = np.zeros(D, dtype=PO.LD)
                e[d] = h
                fd = (p.values(pts.astype(PO.LD) + e) - p.values(pts.astype(PO.LD) - e)) / (2 * h)
                worst = max(worst, float(np.max(np.abs(fd - g[:, :, d])) / np.max(np.abs(g))))
            ism = np.linspace(0.5, 2.0, D)
            assert np.all(p.gradients(pts, ism) == g * ism.astype(PO.LD)[None, None, :])
    print("oracle gradient against central differences: %.3g max |g|" % worst)
    assert worst <= 1e-9


# ---- 2. value and gradient (n_steps = 0) --------------------------------------------------------------------------------------------
def _check_value_cases(ctx, label):
    worst = _Worst()
    for case in CASES:
        pr = _problem(*case)
        g = pr.fit(ctx)
        p = pr.paths(g)
        try:
            r = p.descend(pr.path_of, pr.x0, 0, STEP0, diagnostics=True)
            assert r.flags == 0 and np.all(r.code == 1) and _bits(r.x, pr.x0), case
            assert r.trace.shape == (1, pr.P, 2 * pr.D + 3), case
            # trace row 0 is the evaluation
            assert _bits(r.trace[0, :, :pr.D], pr.x0) and _bits(r.trace[0, :, pr.D], r.value), case
            assert _bits(r.trace[0, :, pr.D + 1:2 * pr.D + 1], r.grad) and np.all(r.trace[0, :, -2] == STEP0), case
            one = _Worst()
            fails = _check_against_oracle(pr, pr.x0, pr.path_of, r.value, r.grad, "%s %r" % (label, case), one)
            print("%s %r: error / bound: value %.3g, gradient %.3g" % (label, case, one.value, one.grad))
            worst.value, worst.grad = max(worst.value, one.value), max(worst.grad, one.grad)
            assert not fails, fails
            # the sweep's values (matrix pipe, dot form) are other bits of the same function: within twice the value bound
            ev = p.evaluate(pr.x0)
            f, _, dev, _ = pr.oracle(pr.x0)
            for i in range(pr.P):
                s = pr.path_of[i]
                o = np.abs(np.asarray(f[s], dtype=np.float64))
                assert abs(ev.values[s, i] - r.value[i]) <= 2 * (MU_RTOL * o[i] + MU_ATOL * max(1.0, o.max()) + 20 * dev[s]), case
        finally:
            p.close()
            g.close()
    print("%s: value cases, largest error / bound: value %.3g, gradient %.3g" % (label, worst.value, worst.grad))


# ---- 3. every step of a trace on its own ---------------------------------------------------------------------------------------------
def _check_traces(ctx, label):
    worst = _Worst()
    for case, T in ((("matern52", 130, 3, 300, 17, 129, 1e-6, False), 30), (("rbf", 65, 17, 65, 64, 17, 1e-2, False), 6)):
        pr = _problem(*case)
        g = pr.fit(ctx)
        p = pr.paths(g)
        try:
            P = 12
            x0, path_of = pr.x0[:P], pr.path_of[:P]
            r = p.descend(path_of, x0, T, STEP0, diagnostics=True)
            D = pr.D
            assert r.trace.shape == (T + 1, P, 2 * D + 3) and _bits(r.trace[0, :, :D], x0)
            xT, fT, gT, steps = GO.replay(r.trace, np.ones(P, dtype=bool), STEP0)
            assert steps == P * T
            # the reported final point, value and gradient are those of the last accepted row
            assert _bits(r.x, xT) and _bits(r.value, fT) and _bits(r.grad, gT)
            assert np.array_equal(r.code, r.trace[-1, :, -1].astype(np.int32))
            # accepted values strictly decrease along every descent
            n_acc = 0
            for i in range(P):
                acc = r.trace[r.trace[:, i, -1] == 1, i, D]
                assert np.all(np.diff(acc) < 0), (i, acc)
                n_acc += acc.size - 1
            assert n_acc >= P                                      # the descents do move
            assert np.all((r.trace[:, :, :D] >= 0.0) & (r.trace[:, :, :D] <= 1.0))
            # value and gradient of every trial point against the oracle at the device's own point
            made = r.trace[:, :, -1] != 2
            tt, ii = np.nonzero(made)
            one = _Worst()
            fails = _check_against_oracle(pr, r.trace[tt, ii, :D], path_of[ii], r.trace[tt, ii, D],
                                          r.trace[tt, ii, D + 1:2 * D + 1], "%s trace %r" % (label, case), one)
            print("%s %r T = %d: %d accepted steps, %d trials; error / bound: value %.3g, gradient %.3g"
                  % (label, case, T, n_acc, tt.size, one.value, one.grad))
            worst.value, worst.grad = max(worst.value, one.value), max(worst.grad, one.grad)
            assert not fails, fails
        finally:
            p.close()
            g.close()
    print("%s: traces, largest error / bound: value %.3g, gradient %.3g" % (label, worst.value, worst.grad))


# ---- 4. edges ----------------------------------------------------------------------------------------------------------------------------
def _descend_raw(L, p, P, path_of, x0, T, step0, null=(), D=None):
    """robo_paths_descend through ctypes with chosen NULL pointers -> the status"""
    D = x0.shape[1] if D is None else D
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    po = np.ascontiguousarray(path_of, dtype=np.int32)
    n = max(P, 1)
    x, v, fl = np.empty((n, D)), np.empty(n), C.c_uint32(0)
    a = dict(p=p, path_of=po.ctypes.data_as(C.POINTER(C.c_int32)), x0=_lib._arr(x0), out_x=_lib._arr(x), out_value=_lib._arr(v),
             out_flags=C.byref(fl))
    for k in null:
        a[k] = None
    st = L.robo_paths_descend(a["p"], P, a["path_of"], a["x0"], T, step0, a["out_x"], a["out_value"], None, None,
                              a["out_flags"], None)
    return st


def _check_edges(ctx, label):
    pr = _problem("matern52", 130, 3, 300, 17, 129, 1e-6, False)
    g = pr.fit(ctx)
    p = pr.paths(g)
    other = _lib.Context(0)
    L = _lib.lib()
    try:
        D, S = pr.D, pr.S
        cand = _lib.Candidates(ctx, pr.x0)
        before = p.evaluate(cand)
        # corners: every (corner, path) evaluated once; a pair whose descent direction points out of the box in every
        # coordinate is frozen at once (codes 1 then 2), one with a single free coordinate moves along it only
        corners = np.array([[(c >> d) & 1 for d in range(D)] for c in range(2 ** D)], dtype=np.float64)
        cx, cs = np.repeat(corners, S, axis=0), np.tile(np.arange(S, dtype=np.int32), 2 ** D)
        r0 = p.descend(cs, cx, 0, STEP0)
        blocked = ((cx <= 0.0) & (r0.grad > 0.0)) | ((cx >= 1.0) & (r0.grad < 0.0))
        full, one_free = np.flatnonzero(blocked.all(axis=1)), np.flatnonzero(blocked.sum(axis=1) == D - 1)
        assert full.size and one_free.size, (full.size, one_free.size)
        i, j = int(full[0]), int(one_free[0])
        r = p.descend(cs[[i, j]], cx[[i, j]], 5, STEP0, diagnostics=True)
        assert r.trace[0, 0, -1] == 1 and np.all(r.trace[1:, 0, -1] == 2) and r.flags & _lib.FLAG_FROZEN
        assert _bits(r.x[0], cx[i]) and _bits(r.value[0], r0.value[i]) and _bits(r.trace[1:, 0, :D], np.tile(cx[i], (5, 1)))
        free = int(np.flatnonzero(~blocked[j])[0])
        assert r.trace[1, 1, -1] in (0, 1) and r.trace[1, 1, free] != cx[j, free]
        assert _bits(np.delete(r.trace[1, 1, :D], free), np.delete(cx[j], free))
        GO.replay(r.trace, np.ones(2, dtype=bool), STEP0)
        # P = 1, n_steps = 0; and the same point in a batch gives the same bits
        r1 = p.descend(pr.path_of[5:6], pr.x0[5:6], 0, STEP0)
        rall = p.descend(pr.path_of, pr.x0, 0, STEP0)
        assert _bits(r1.value, rall.value[5:6]) and _bits(r1.grad, rall.grad[5:6]) and r1.code[0] == 1
        # a path whose weights are finite and whose value is not: code 3 at the start, the flag, nothing evolves
        big = g.sample_paths(pr.omega, pr.phase, pr.w[:2] * 1e307, pr.eps[:2])      # (max |w| = 3.3: finite)
        try:
            rb = big.descend(np.array([0, 1], dtype=np.int32), pr.x0[:2], 4, STEP0, diagnostics=True)
            assert not np.isfinite(rb.value).any() and rb.flags & _lib.FLAG_FROZEN
            assert np.all(rb.trace[0, :, -1] == 3) and np.all(rb.trace[1:, :, -1] == 2) and _bits(rb.x, pr.x0[:2])
            assert np.all(rb.code == 2)
        finally:
            big.close()
        assert p.descend(pr.path_of[:3], pr.x0[:3], 2, STEP0).flags & ~_lib.FLAG_FROZEN == 0       # the flag does not stick
        # refusals of robo_paths_descend: the status, a reason, nothing launched
        po, x0 = pr.path_of[:4].copy(), pr.x0[:4].copy()

        def refused(want, *a, **kw):
            st = _descend_raw(L, *a, **kw)
            assert st == want and len(_lib.last_error()) > 0, (st, want, _lib.last_error())
        for bad in (-1e-300, 1.0 + 1e-15, np.nan, np.inf, -np.inf):
            xb = x0.copy()
            xb[2, 1] = bad
            refused(_lib.BAD_ARGUMENT, p._h, 4, po, xb, 3, STEP0)
        for bad in (-1, S):
            pb = po.copy()
            pb[3] = bad
            refused(_lib.BAD_ARGUMENT, p._h, 4, pb, x0, 3, STEP0)
        refused(_lib.BAD_ARGUMENT, p._h, 0, po, x0, 3, STEP0)
        refused(_lib.BAD_ARGUMENT, p._h, _lib.PATHS_MAX_DESCENTS + 1, po, x0, 3, STEP0)
        refused(_lib.BAD_ARGUMENT, p._h, 4, po, x0, -1, STEP0)
        for bad in (0.0, -0.1, 0.5 + 1e-12, np.nan):
            refused(_lib.BAD_ARGUMENT, p._h, 4, po, x0, 3, bad)
        for k in ("p", "path_of", "x0", "out_x", "out_value", "out_flags"):
            refused(_lib.BAD_ARGUMENT, p._h, 4, po, x0, 3, STEP0, null=(k,))
        with pytest.raises(_lib.RoboBadShape):
            p.descend(po, x0[:, :2], 1, STEP0)
        # refusals of robo_paths_refine_cand
        wide = _lib.Candidates(ctx, np.random.RandomState(0).rand(5, D + 1))
        far = _lib.Candidates(other, pr.x0[:5])
        try:
            with pytest.raises(_lib.RoboBadShape):
                p.refine(wide, 4, 2, STEP0)
            with pytest.raises(ValueError, match="context"):
                p.refine(far, 4, 2, STEP0)
            for K in (0, _lib.PATHS_MAX_STARTS + 1):
                with pytest.raises(ValueError):
                    p.refine(cand, K, 2, STEP0, diagnostics=True)
            for T, a0 in ((-1, STEP0), (2, 0.0), (2, 0.6)):
                with pytest.raises(ValueError):
                    p.refine(cand, 4, T, a0)
            x, v, si, fl = np.empty((S, D)), np.empty(S), np.empty(S, dtype=np.int64), C.c_uint32(0)
            i64 = si.ctypes.data_as(C.POINTER(C.c_int64))
            for a in ((None, cand._h, 4, 2, STEP0, _lib._arr(x), _lib._arr(v), i64, C.byref(fl), None, None),
                      (p._h, None, 4, 2, STEP0, _lib._arr(x), _lib._arr(v), i64, C.byref(fl), None, None),
                      (p._h, cand._h, 4, 2, STEP0, None, _lib._arr(v), i64, C.byref(fl), None, None),
                      (p._h, cand._h, 4, 2, STEP0, _lib._arr(x), None, i64, C.byref(fl), None, None),
                      (p._h, cand._h, 4, 2, STEP0, _lib._arr(x), _lib._arr(v), None, C.byref(fl), None, None),
                      (p._h, cand._h, 4, 2, STEP0, _lib._arr(x), _lib._arr(v), i64, None, None, None)):
                assert L.robo_paths_refine_cand(*a) == _lib.BAD_ARGUMENT and len(_lib.last_error()) > 0
        finally:
            wide.close()
            far.close()
        # the object gives the same robo_paths_eval_cand bits afterwards
        after = p.evaluate(cand)
        assert _bits(after.values, before.values) and _bits(after.min, before.min) and np.array_equal(after.argmin, before.argmin)
        assert after.flags == 0
        cand.close()
    finally:
        other.close()
        p.close()
        g.close()
    # dim = 1 and N = 1 with steps: the rule holds on the trace
    for case in (("rbf", 63, 1, 63, 2, 17, 1e-6, True), ("rbf", 1, 1, 300, 1, 17, 1e-6, False),
                 ("matern52", 1, 1, 1, 1, 1, 1e-2, False)):
        pr = _Problem(*case)
        g = pr.fit(ctx)
        p = pr.paths(g)
        try:
            r = p.descend(pr.path_of, pr.x0, 8, STEP0, diagnostics=True)
            xT, fT, gT, _ = GO.replay(r.trace, np.ones(pr.P, dtype=bool), STEP0)
            assert _bits(r.x, xT) and _bits(r.value, fT) and _bits(r.grad, gT)
            assert np.all(r.value <= r.trace[0, :, pr.D])
        finally:
            p.close()
            g.close()
    # above the stated bound of 64 dimensions: ROBO_BAD_SHAPE before anything is launched
    rs = np.random.RandomState(3)
    Dw, Nw, Fw = 65, 8, 4
    gw = _lib.DeviceGP(ctx, "rbf", Nw, Dw)
    gw.set_data(rs.rand(Nw, Dw), rs.randn(Nw))
    gw.fit(np.concatenate([[0.0], np.zeros(Dw), [np.log(1e-2)]]), 0.0)
    pw = gw.sample_paths(*draw_features("rbf", Dw, Fw, rs), rs.standard_normal((1, Fw)), rs.standard_normal((1, Nw)))
    cw = _lib.Candidates(ctx, rs.rand(3, Dw))
    try:
        with pytest.raises(_lib.RoboBadShape):
            pw.descend(np.zeros(3, dtype=np.int32), rs.rand(3, Dw), 1, STEP0)
        with pytest.raises(_lib.RoboBadShape):
            pw.refine(cw, 2, 1, STEP0)
        assert pw.evaluate(cw).flags == 0
    finally:
        cw.close()
        pw.close()
        gw.close()


# ---- 5. invariances, bit for bit ------------------------------------------------------------------------------------------------------
def _check_invariances(ctx, label):
    pr = _problem("matern52", 130, 3, 300, 17, 129, 1e-6, False)
    g = pr.fit(ctx)
    rs = np.random.RandomState(11)
    p = pr.paths(g)
    T, s, x = 9, 5, pr.x0[7:8]
    try:
        base = p.descend(np.array([s], dtype=np.int32), x, T, STEP0, diagnostics=True)           # slot 0 of P = 1
        # in the middle of P = 129, among other paths' descents, sharing its workgroup with them
        x0, po = pr.x0.copy(), pr.path_of.copy()
        x0[66], po[66] = x[0], s
        mid = p.descend(po, x0, T, STEP0, diagnostics=True)
        assert _bits(mid.trace[:, 66], base.trace[:, 0]) and _bits(mid.x[66], base.x[0]) and _bits(mid.value[66:67], base.value)
        # at another place of its workgroup, next to frozen neighbours
        x3 = np.array([x[0], [0.0] * pr.D, x[0]])
        r3 = p.descend(np.array([s, s, s], dtype=np.int32), x3, T, STEP0, diagnostics=True)
        assert _bits(r3.trace[:, 0], base.trace[:, 0]) and _bits(r3.trace[:, 2], base.trace[:, 0])
        # a paths object with S = 1 holding only that path's draws, and one with S = 64 and other draws around it
        p1 = pr.paths(g, slice(s, s + 1))
        w64, e64 = rs.standard_normal((64, pr.F)), rs.standard_normal((64, pr.N))
        w64[40], e64[40] = pr.w[s], pr.eps[s]
        p64 = g.sample_paths(pr.omega, pr.phase, w64, e64)
        try:
            a = p1.descend(np.array([0], dtype=np.int32), x, T, STEP0, diagnostics=True)
            b = p64.descend(np.array([3, 40, 63], dtype=np.int32), np.repeat(x, 3, axis=0), T, STEP0, diagnostics=True)
            assert _bits(a.trace, base.trace) and _bits(b.trace[:, 1], base.trace[:, 0])
            assert not _bits(b.trace[:, 0], base.trace[:, 0])
        finally:
            p1.close()
            p64.close()
        # the fused call's starts fed back to the explicit entry point
        cand = _lib.Candidates(ctx, rs.rand(401, pr.D))
        try:
            K = 5
            rf = p.refine(cand, K, T, STEP0, diagnostics=True)
            used = rf.starts.ravel() >= 0
            assert used.all()
            pts = np.array([cand.point(int(i)) for i in rf.starts.ravel()])
            rd = p.descend(np.repeat(np.arange(pr.S, dtype=np.int32), K), pts, T, STEP0, diagnostics=True)
            assert _bits(rd.trace, rf.trace)
        finally:
            cand.close()
    finally:
        p.close()
        g.close()


# ---- 6. selection and the fused form ---------------------------------------------------------------------------------------------------
def _check_fused(ctx, label):
    pr = _problem("matern52", 65, 3, 65, 17, 129, 1e-2, False)
    g = pr.fit(ctx)
    p = pr.paths(g)
    rs = np.random.RandomState(21)
    K, T, D, S = 3, 7, pr.D, pr.S
    try:
        pool = rs.rand(401, D)

        def one(Xc, K=K, T=T, tie=False):
            cand = _lib.Candidates(ctx, Xc)
            try:
                before = p.evaluate(cand)
                rf = p.refine(cand, K, T, STEP0, diagnostics=True)
                after = p.evaluate(cand)
                assert _bits(after.values, before.values) and _bits(after.min, before.min) and after.flags == before.flags
                want = np.array([GO.group_starts(before.values[s], K) for s in range(S)])
                assert np.array_equal(rf.starts, want), (Xc.shape, rf.starts, want)
                used = (rf.starts >= 0).ravel()
                # unused slots: code 2 in every row of the trace, never evolved
                assert np.all(rf.trace[:, ~used, -1] == 2)
                pts = np.where(used[:, None], Xc[np.maximum(rf.starts.ravel(), 0)], 0.0)
                assert _bits(rf.trace[0, :, :D][used], pts[used])
                xT, fT, gT, _ = GO.replay(rf.trace, used, STEP0)
                # each path's winner is the smallest final value of its own descents, first slot on ties
                for s in range(S):
                    f = np.where(used[s * K:(s + 1) * K], fT[s * K:(s + 1) * K], np.inf)
                    if not used[s * K:(s + 1) * K].any():
                        assert rf.start_index[s] == -1 and np.isnan(rf.value[s])
                        continue
                    k = int(np.argmin(f))
                    assert _bits(rf.value[s:s + 1], f[k:k + 1]) and rf.start_index[s] == rf.starts[s, k], (s, f, rf.value[s])
                    assert _bits(rf.x[s], xT[s * K + k])
                # n_steps = 0: the sweep's own pick, point and value
                r0 = p.refine(cand, K, 0, STEP0)
                has = rf.starts[:, 0] >= 0
                clean = ~np.isnan(before.values).any()
                if clean:
                    assert np.array_equal(r0.start_index, before.argmin) and _bits(r0.value, before.min)
                    assert _bits(r0.x, Xc[before.argmin]) and r0.flags == before.flags
                assert np.array_equal(r0.start_index[has], rf.starts[has, 0])
                return before, rf
            finally:
                cand.close()
        for m in (1, 63, 64, 65, 64 * K + 1, 401):
            one(pool[:m])
        # n_starts larger than the number of groups
        _, rf = one(pool[:130], K=5)
        assert np.all(rf.starts[:, 3:] == -1) and np.all(rf.starts[:, :3] >= 0)
        # equal values in two groups: path 0's best row copied into another group -- the earlier row comes first
        ev, _ = one(pool[:193])
        b = int(ev.argmin[0])
        Xt = pool[:193].copy()
        c = (b + 64) % 192
        Xt[c] = Xt[b]
        ev2, rf2 = one(Xt)
        assert ev2.values[0, b] == ev2.values[0, c] and sorted(rf2.starts[0, :2].tolist()) == sorted([b, c])
        assert rf2.starts[0, 0] == min(b, c)
        # a NaN candidate loses its group
        Xn = pool[:193].copy()
        Xn[b, 1] = np.nan
        evn, rfn = one(Xn)
        assert rfn.flags & _lib.FLAG_NAN and not np.any(rfn.starts // 64 == b // 64) and np.isnan(evn.min).all()
        assert np.all(np.isfinite(rfn.value))
        # an all-NaN batch: no start, a NaN value
        cand = _lib.Candidates(ctx, np.full((70, D), np.nan))
        try:
            ra = p.refine(cand, K, T, STEP0, diagnostics=True)
            assert np.all(ra.start_index == -1) and np.isnan(ra.value).all() and ra.flags & _lib.FLAG_NAN
            assert np.all(ra.starts == -1) and np.all(ra.trace[:, :, -1] == 2)
            r0 = p.refine(cand, K, 0, STEP0)
            assert np.all(r0.start_index == -1) and np.isnan(r0.value).all()
        finally:
            cand.close()
        assert p.evaluate(pool[:70]).flags == 0
        # a workspace so small that the sweep runs in several chunks gives the same starts and the same trajectories
        cand = _lib.Candidates(ctx, pool)
        try:
            whole = p.refine(cand, K, T, STEP0, diagnostics=True)
            n_pad = (pr.N + 1 + 127) // 128 * 128
            ctx.set_tuning("ws_bytes", 128 * n_pad * 8)
            try:
                parts = p.refine(cand, K, T, STEP0, diagnostics=True)
            finally:
                ctx.set_tuning("ws_bytes", None)
            assert 401 > 3 * 128 and np.array_equal(parts.starts, whole.starts) and _bits(parts.trace, whole.trace)
            assert _bits(parts.value, whole.value) and _bits(parts.x, whole.x)
        finally:
            cand.close()
    finally:
        p.close()
        g.close()


# ---- 7. it finds the minimum --------------------------------------------------------------------------------------------------------------
_MIN = dict(kind="matern52", N=40, D=2, F=300, S=4, m=300, K=16, T=40, seed=6)


def _bowl(X):
    """a target whose minimum lies inside the box, so that the paths' minimisers are no grid points"""
    return 4.0 * np.sum((X - 0.45) ** 2, axis=1) + 0.3 * np.sin(9.0 * X[:, 0])


def _check_minimum(ctx, label):
    """D = 2, N = 40, F = 300, S = 4, 300 candidates, n_starts = 16, T = 40.  The yardstick is the minimum of the long-double
    oracle over a 129 x 129 grid of the box (spacing 1/128: a grid point lies within 0.0055 of the minimiser).  T = 40 was
    chosen on the CPU: the fp64 restatement of the rule on the oracle's value and gradient (np.float64), from the group
    rule's starts on the oracle's own sweep values, ends below the grid minimum for every path -- asserted here first --
    and then the same is asserted of the device.  Gap closure (sweep's best - result) / (sweep's best - grid minimum), the
    smallest over the four paths: restatement 1.0088, interpreter 1.0088, MI355X 1.0088 (the restatement ends 1.7e-5 to
    2.4e-4 below the grid minimum; the bowl-shaped target puts the minimisers inside the box, off the grid)."""
    z = _MIN
    pr = _Problem(z["kind"], z["N"], z["D"], z["F"], z["S"], z["m"], 1e-2, True, seed=z["seed"], target=_bowl)
    Xc = np.random.RandomState(66).rand(z["m"], z["D"])
    t = np.linspace(0.0, 1.0, 129)
    grid = np.array([[a, b] for a in t for b in t])
    grid_min = np.min(pr.model(PO.LD).values(CO.scale(grid, pr.lnm)), axis=1).astype(np.float64)          # (S,)
    m64 = pr.model(np.float64)
    sweep = m64.values(CO.scale(Xc, pr.lnm))
    closure_cpu = []
    for s in range(z["S"]):
        def fn(x, s=s):
            xs = CO.scale(x[None, :], pr.lnm)
            return float(m64.values(xs)[s, 0]), np.asarray(m64.gradients(xs, pr.ism)[s, 0], dtype=np.float64)
        ends = [GO.descend(fn, Xc[i], z["T"], STEP0)[1] for i in GO.group_starts(sweep[s], z["K"]) if i >= 0]
        assert min(ends) < grid_min[s] - 1e-6, (s, min(ends), grid_min[s])      # room to spare: fp64 noise is 1e-14 here
        closure_cpu.append((sweep[s].min() - min(ends)) / (sweep[s].min() - grid_min[s]))
    g = pr.fit(ctx)
    p = pr.paths(g)
    cand = _lib.Candidates(ctx, Xc)
    try:
        ev = p.evaluate(cand, want_values=False)
        r = p.refine(cand, z["K"], z["T"], STEP0)
        closure = (ev.min - r.value) / (ev.min - grid_min)
        print("%s: gap closure, restatement %.4f, device %.4f (smallest over %d paths)"
              % (label, min(closure_cpu), closure.min(), z["S"]))
        assert np.all(r.value < grid_min), (r.value, grid_min)
        assert np.all((r.x >= 0.0) & (r.x <= 1.0)) and np.all(r.value < ev.min)
    finally:
        cand.close()
        p.close()
        g.close()


# ---- 8. the classes and the front end -------------------------------------------------------------------------------------------------------
_BOX = (np.array([-5.0, 0.0]), np.array([10.0, 15.0]))


def _branin(x):
    x = np.asarray(x, dtype=np.float64)
    return float((x[1] - 5.1 / (4 * np.pi ** 2) * x[0] ** 2 + 5.0 / np.pi * x[0] - 6.0) ** 2
                 + 10.0 * (1.0 - 1.0 / (8 * np.pi)) * np.cos(x[0]) + 10.0)


def _data(n, seed):
    rs = np.random.RandomState(seed)
    X = _BOX[0] + (_BOX[1] - _BOX[0]) * rs.rand(n, 2)
    return rs, X, np.array([_branin(x) for x in X]) / 50.0


def _gp_model(**kw):
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models import GaussianProcess
    rs, X, y = _data(14, 0)
    model = GaussianProcess(2 * Matern52Kernel(np.array([0.5, 0.8]), ndim=2), noise=1e-3, lower=_BOX[0], upper=_BOX[1], **kw)
    model.train(X, y, do_optimize=False)
    return rs, model


def _mcmc_model():
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models.gaussian_process_mcmc import GaussianProcessMCMC
    from robo_amd.priors.default_priors import DefaultPrior
    rs, X, y = _data(10, 2)
    kernel = 2 * Matern52Kernel(np.ones(2), ndim=2)
    model = GaussianProcessMCMC(kernel, prior=DefaultPrior(len(kernel) + 1, rng=np.random.RandomState(3)), n_hypers=8,
                                chain_length=4, burnin_steps=2, rng=np.random.RandomState(4), lower=_BOX[0], upper=_BOX[1])
    model.train(X, y)
    return rs, model


def _replay_path0(model, seed, n_paths, n_features):
    """the draws of ThompsonSampling._draw from the same seed -> (the sub-model behind path 0, its GradPaths in long double
    and fp64 holding the group's paths, path 0's number in the group)"""
    subs = list(model.models) if hasattr(model, "models") else [model]
    rs = np.random.RandomState(seed)
    idx = np.array([rs.randint(len(subs)) for _ in range(n_paths)]) if len(subs) > 1 else np.zeros(n_paths, dtype=np.int64)
    for i in sorted(set(idx.tolist())):
        sub = subs[i]
        members = np.flatnonzero(idx == i)
        theta = np.asarray(_lib._full_theta(sub.gp, sub._fitted_theta), dtype=np.float64)
        D, N = sub.X.shape[1], sub.X.shape[0]
        omega, phase = draw_features(sub.kernel.kind, D, n_features, rs)
        w, eps = rs.standard_normal((len(members), n_features)), rs.standard_normal((len(members), N))
        if 0 in members:
            ym, ys = (sub.y_mean, sub.y_std) if sub.normalize_output else (0.0, 1.0)
            mk = lambda dt: GO.GradPaths(sub.kernel.kind, float(np.exp(theta[0])), float(np.exp(theta[-1])),  # noqa: E731
                                         CO.scale(sub.X, theta[1:-1]), sub.y, float(sub.mean), omega, phase, w, eps, ym, ys,
                                         dtype=dt)
            return sub, theta, mk(PO.LD), mk(np.float64), int(np.flatnonzero(members == 0)[0])
    raise AssertionError("no group holds path 0")


def _check_class(ctx, label):
    from robo_amd.acquisition_functions import EI, MES, ThompsonSampling
    from robo_amd.maximizers import DeviceGradientAscent
    span = _BOX[1] - _BOX[0]
    for (rs, model), n_paths, seed in ((_gp_model(), 6, 31), (_mcmc_model(), 9, 32)):
        acq = ThompsonSampling(model, n_paths=n_paths, n_features=64, rng=np.random.RandomState(seed))
        acq.update(model)
        Xc = _BOX[0] + span * rs.rand(150, 2)
        K, T = 2, 12
        x = acq.refine(Xc, n_starts=K, n_steps=T, step0=STEP0, diagnostics=True)
        res = acq.last_refine
        sub, theta, orc, m64, at = _replay_path0(model, seed, n_paths, 64)
        assert x.shape == (2,) and np.all(x >= _BOX[0]) and np.all(x <= _BOX[1])
        assert _bits(x, _BOX[0] + span * res.x[at]) and _bits([acq.last_max], [-res.value[at]])
        assert acq.last_argmax == res.start_index[at] and acq.last_argmax in res.starts[at]
        # path 0's descents replayed through the oracle: every trial point's value and gradient, and the rule
        tr = res.trace[:, at * K:(at + 1) * K]
        used = res.starts[at] >= 0
        xT, fT, _, _ = GO.replay(tr, used, STEP0)
        k = int(np.argmin(np.where(used, fT, np.inf)))
        assert _bits(res.value[at:at + 1], fT[k:k + 1]) and _bits(res.x[at], xT[k])
        pts = tr[:, used, :2].reshape(-1, 2)
        ism = CO.inv_sqrt_metric(theta[1:-1])
        Xs = CO.scale(pts, theta[1:-1])
        f, g = orc.values(Xs)[at], orc.gradients(Xs, ism)[at]
        dev = float(np.max(np.abs(m64.values(Xs)[at] - f)))
        dev_g = float(np.max(np.abs(m64.gradients(Xs, ism)[at] - g)))
        o = np.abs(np.asarray(f, dtype=np.float64))
        bound = MU_RTOL * o + MU_ATOL * max(1.0, float(o.max())) + 20.0 * dev
        err = np.abs(tr[:, used, 2].ravel().astype(PO.LD) - f).astype(np.float64)
        gerr = float(np.max(np.abs(tr[:, used, 3:5].reshape(-1, 2).astype(PO.LD) - g)))
        gb = 1e-13 * float(np.max(np.abs(g))) + 20.0 * dev_g
        print("%s: class %s replay: error / bound: value %.3g, gradient %.3g"
              % (label, type(model).__name__, float(np.max(err / bound)), gerr / gb))
        assert np.all(err <= bound) and gerr <= gb
        # the starts are rows of the candidates, in the normalised box
        assert _bits(tr[0, used, :2], sub._normalised(Xc)[res.starts[at][used]])
        # a device batch in the normalised box is the same call
        cand = _lib.Candidates(sub.gp.ctx, sub._normalised(Xc))
        try:
            assert _bits(acq.refine(cand, n_starts=K, n_steps=T, step0=STEP0), x)
        finally:
            cand.close()
        # select_batch: refine=False is today's result; refine=True is one refined point per path, duplicates kept
        plain = acq.select_batch(Xc, 4)
        rows = acq.last_batch.copy()
        assert _bits(plain, Xc[rows]) and _bits(acq.select_batch(Xc, 4, refine=False, n_starts=K), plain)
        pts = acq.select_batch(Xc, 4, refine=True, n_starts=K, n_steps=T, step0=STEP0)
        assert pts.shape == (4, 2) and np.all(pts >= _BOX[0]) and np.all(pts <= _BOX[1]) and acq.last_batch.shape == (4,)
        assert _bits(pts[0], x) and np.all(acq.last_batch >= 0)
        vals, _, _ = acq._evaluate(Xc, True)
        got, _ = acq.value_and_gradient(pts)          # (path 0 at all four points: only the first is its own)
        assert -got[0] <= vals[0].min() + 1e-9
        for j in range(4):                                   # every point is its own path's refined minimiser
            grp, a = acq._group_of(j)
            rj = grp.descend(np.array([a], dtype=np.int32), sub._normalised(pts[j:j + 1]), 0, STEP0)
            assert rj.value[0] <= vals[j].min() + 1e-9 * max(1.0, abs(vals[j].min()))
        # value_and_gradient: shapes, one consistent function, central differences through the normalisation (lower != 0,
        # upper - lower != 1)
        Xq = _BOX[0] + span * (0.1 + 0.8 * rs.rand(7, 2))
        f, df = acq.value_and_gradient(Xq)
        assert f.shape == (7,) and df.shape == (7, 2)
        plain_f = acq.compute(Xq)
        assert np.all(np.abs(f - plain_f) <= 1e-9 * np.maximum(1.0, np.abs(plain_f)))
        for d in range(2):
            h = 1e-5 * span[d]
            e = np.zeros(2)
            e[d] = h
            fd = (acq.value_and_gradient(Xq + e)[0] - acq.value_and_gradient(Xq - e)[0]) / (2 * h)
            # h^2 f''' / 6 + eps |f| / h: both below 1e-6 of the gradient's scale here
            assert np.all(np.abs(fd - df[:, d]) <= 1e-6 * np.max(np.abs(df)) + 1e-9), (d, fd, df[:, d])
        # the maximiser: a Thompson objective is refined; anything else without a closed form still is not
        np.random.seed(4)
        mx = DeviceGradientAscent(acq, _BOX[0], _BOX[1], n_samples=128, n_starts=2, n_steps=5, rng=np.random.RandomState(9))
        xm = mx.maximize()
        assert xm.shape == (2,) and np.all(xm >= _BOX[0]) and np.all(xm <= _BOX[1])
        xb = mx.maximize_batch(3)
        assert xb.shape == (3, 2) and np.all(xb >= _BOX[0]) and np.all(xb <= _BOX[1])
        assert not hasattr(DeviceGradientAscent(EI(model), _BOX[0], _BOX[1]), "maximize_batch")
        with pytest.raises(TypeError, match="has no gradient on the device"):
            DeviceGradientAscent(MES(model), _BOX[0], _BOX[1], n_samples=64).maximize()
        sub.devices = [0, 1]
        try:
            for call in (lambda: acq.refine(Xc), lambda: acq.select_batch(Xc, 2, refine=True),
                         lambda: acq.value_and_gradient(Xc), lambda: mx.maximize()):
                with pytest.raises(NotImplementedError):
                    call()
        finally:
            sub.devices = None
        with pytest.raises(NotImplementedError):
            acq.refine(_lib.CandidateShards([], []))
    # the model checks of the refinement: normalize_input=True
    rs, raw = _gp_model(normalize_input=False)
    acq = ThompsonSampling(raw, n_paths=2, n_features=32, rng=np.random.RandomState(1))
    with pytest.raises(TypeError, match="normalize_input"):
        acq.refine(rs.rand(20, 2))
    with pytest.raises(TypeError, match="normalize_input"):
        DeviceGradientAscent(acq, _BOX[0], _BOX[1], n_samples=64).maximize()


def _check_front_end(ctx):
    from robo_amd.fmin import bayesian_optimization

    def run(seed, **kw):
        np.random.seed(seed)
        calls = []

        def f(x):
            calls.append(np.array(x))
            return _branin(x)
        kw.setdefault("model_type", "gp")
        res = bayesian_optimization(f, _BOX[0], _BOX[1], acquisition_func="thompson", maximizer="device_gradient", n_init=3,
                                    n_candidates=128, rng=np.random.RandomState(seed), n_features=64, **kw)
        X = np.array(res["X"])
        assert X.shape[0] == len(calls) and np.all(X >= _BOX[0]) and np.all(X <= _BOX[1]) and np.all(np.isfinite(res["y"]))
        return X
    X = run(1, num_iterations=6)
    assert X.shape == (6, 2) and len({tuple(x) for x in X}) == 6
    assert _bits(run(1, num_iterations=6), X)                                        # reproducible from the seed
    assert not _bits(run(2, num_iterations=6), X)
    X = run(1, num_iterations=9, batch_size=3)
    assert X.shape == (9, 2) and _bits(run(1, num_iterations=9, batch_size=3), X)
    X = run(3, num_iterations=5, model_type="gp_mcmc", chain_length=4, burnin_steps=2)
    assert X.shape == (5, 2)


# ---- the runs --------------------------------------------------------------------------------------------------------------------------
def test_values_and_gradients_emu(emu_ctx):
    _check_value_cases(emu_ctx, "interpreter")


def test_traces_emu(emu_ctx):
    _check_traces(emu_ctx, "interpreter")


def test_edges_emu(emu_ctx):
    _check_edges(emu_ctx, "interpreter")


def test_invariances_emu(emu_ctx):
    _check_invariances(emu_ctx, "interpreter")


def test_fused_emu(emu_ctx):
    _check_fused(emu_ctx, "interpreter")


def test_minimum_emu(emu_ctx):
    _check_minimum(emu_ctx, "interpreter")


def test_class_emu(emu_ctx):
    _check_class(emu_ctx, "interpreter")


def test_front_end_emu(emu_ctx):
    _check_front_end(emu_ctx)


@pytest.mark.gpu
def test_values_and_gradients_gpu(gpu_ctx):
    _check_value_cases(gpu_ctx, "MI355X")


@pytest.mark.gpu
def test_traces_gpu(gpu_ctx):
    _check_traces(gpu_ctx, "MI355X")


@pytest.mark.gpu
def test_edges_and_invariances_gpu(gpu_ctx):
    _check_edges(gpu_ctx, "MI355X")
    _check_invariances(gpu_ctx, "MI355X")


@pytest.mark.gpu
def test_fused_gpu(gpu_ctx):
    _check_fused(gpu_ctx, "MI355X")


@pytest.mark.gpu
def test_minimum_gpu(gpu_ctx):
    _check_minimum(gpu_ctx, "MI355X")


@pytest.mark.gpu
def test_class_and_front_end_gpu(gpu_ctx):
    _check_class(gpu_ctx, "MI355X")
    _check_front_end(gpu_ctx)
