"""Two-objective expected hypervolume improvement (robo_amd/csrc/ehvi.hip, api_ehvi.hip: robo_ehvi_eval_cand,
robo_ehvi_eval_moments; util/pareto.py, the EHVI class and the multi_objective_optimization front end) against
tests/ehvi_oracle.py.

CPU: through the interpreter (tests/hipemu).  -m gpu: the same checks at the same small shapes on the MI355X, plus the fused
form at N = 256, D = 4, m = 32 773, P = 50.

The oracle is the strip rule in np.longdouble, itself checked against the exact gain of deterministic points and against a
product trapezoid rule (test_oracle).

The value bound.  The device value is compared with the oracle fed THE DEVICE'S OWN DOUBLES (the trace, or the inputs of the
moments form); per candidate

    |EHVI_dev - EHVI_orc| <= 28 eps unit + floor

with unit, the count behind 28 (13.6 doubled) and the floor (what the cut at |z| > 36 may cost: below 1e-284 of the factors)
derived in tests/ehvi_oracle.py.  The kernel reads the front through uniform loads, front point by front point: there is
no staging tile and so no tile edge beyond the listed P.  Largest observed error / (eps unit):
    interpreter:   1.48 (moments groups), 1.59 (chosen cases), 2.22 (fused cases)
    MI355X:        1.03 (moments groups), 1.34 (chosen cases), 1.59 (fused cases), 0.89 (fused large)
"""
import copy
import os
import sys

import numpy as np
import pytest

from robo_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ehvi_oracle as EO  # noqa: E402
from _tol import ACQ_RTOL  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402

LD = EO.LD
EPS = np.finfo(np.float64).eps
REF = np.array([1.1, 1.1])
TINY = 1e-12 * 1.21
PS = (0, 1, 2, 63, 64, 65, 257)
MS = (1, 63, 64, 65, 400, 401)
SMALL = dict(N=80, D=3, Ms=(400, 401))
LARGE = dict(N=256, D=4, M=32768 + 5, P=50)


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


def _curve_front(rs, P, scale=1.0):
    t = np.sort(rs.rand(P))
    return np.stack((t, 1.0 - np.sqrt(t)), axis=1) * scale


class _Worst(object):
    ratio = 0.0


_ORACLE = {}


def _oracle(key, mu1, v1, mu2, v2, front, ref):
    """ehvi_oracle on these doubles, computed once per key and shared between the interpreter and the MI355X runs"""
    if key is None or key not in _ORACLE:
        out = EO.ehvi_batch(mu1, v1, mu2, v2, front, ref)
        if key is None:
            return out
        for a in out:
            a.setflags(write=False)
        _ORACLE[key] = (out, np.array(mu1).tobytes() + np.array(v1).tobytes() + np.array(mu2).tobytes() + np.array(v2).tobytes())
    out, stamp = _ORACLE[key]
    assert stamp == np.array(mu1).tobytes() + np.array(v1).tobytes() + np.array(mu2).tobytes() + np.array(v2).tobytes(), key
    return out


def _check_values(vals, orc, label, worst, rows=None):
    """every (listed) candidate's value against the oracle on the same doubles, within the bound; values >= 0"""
    total, unit, floor = orc
    rows = np.arange(len(vals)) if rows is None else np.asarray(rows)
    for k, c in enumerate(rows):
        if np.isnan(total[k]):
            assert np.isnan(vals[c]), (label, c)
            continue
        err = abs(LD(vals[c]) - total[k])
        if unit[k] > 0 and err > floor[k]:
            worst.ratio = max(worst.ratio, float((err - floor[k]) / (LD(EPS) * unit[k])))
        assert vals[c] >= 0.0 and err <= EO.bound(unit[k], floor[k]), \
            (label, int(c), vals[c], float(total[k]), float(err), float(EO.bound(unit[k], floor[k])))


# ---- the oracle itself and the host helpers ---------------------------------------------------------------------------------
def test_oracle():
    """the strip rule in np.longdouble against (a) the exact hypervolume gain of deterministic points (s = 0), from
    hypervolume_2d before and after, (b) a product trapezoid rule (1601 x 1601 nodes on +-10 s) of HVI(y) phi phi.
    Worst relative difference to the quadrature observed: 3.3e-6 (the integrand has kinks: the rule is O(h^2))."""
    from robo_amd.util.pareto import hypervolume_2d, pareto_front_2d
    rs = np.random.RandomState(1)
    worst = 0.0
    for P in (0, 1, 2, 6):
        front = _curve_front(rs, P)
        before = hypervolume_2d(front, REF)
        for _ in range(30):
            y = rs.rand(2) * 1.3 - 0.1
            after = hypervolume_2d(pareto_front_2d(np.concatenate((front, y[None])), REF)[0], REF)
            got = float(EO.ehvi(y[0], 0.0, y[1], 0.0, front, REF)[0])
            assert abs(got - (after - before)) <= 1e-14, (P, y, got, after - before)
            assert abs(float(EO.hvi(y[:1], y[1:], front, REF)[0]) - (after - before)) <= 1e-14
        for _ in range(2):
            mu, s = rs.rand(2) * 1.1, 0.055 + rs.rand(2)
            val = float(EO.ehvi(mu[0], s[0] ** 2, mu[1], s[1] ** 2, front, REF)[0])
            q = EO.quadrature(mu[0], s[0] ** 2, mu[1], s[1] ** 2, front, REF)
            worst = max(worst, abs(val - q) / val)
            assert abs(val - q) <= 2e-5 * val, (P, val, q)
    print("oracle against quadrature: worst relative difference %.3e" % worst)
    # f without the cut continues f with it; its tail obeys the bound the floor is built on
    assert abs(float(EO.f_tail(36.0)[0] / EO.KO.f_tail(36.0)[0]) - 1.0) < 1e-17
    t = np.array([36.5, 38.0])
    assert np.all(EO.f_tail(t) > 0) and np.all(EO.f_tail(t) < EO._PHI_CUT)


def _brute_front(Y, ref):
    """O(N^2): indices of the points strictly inside ref that no other point dominates or duplicates at a lower index"""
    keep = []
    for i, y in enumerate(Y):
        if not (y[0] < ref[0] and y[1] < ref[1]):
            continue
        dominated = False
        for j, w in enumerate(Y):
            if j == i or not (w[0] < ref[0] and w[1] < ref[1]):
                continue
            if (w[0] <= y[0] and w[1] <= y[1]) and ((w[0] < y[0] or w[1] < y[1]) or j < i):
                dominated = True
        if not dominated:
            keep.append(i)
    return sorted(keep, key=lambda i: Y[i, 0])


def test_pareto_helpers():
    from robo_amd.util.pareto import exclusive_contributions_2d, hypervolume_2d, pareto_front_2d
    rs = np.random.RandomState(2)
    for case in range(40):
        n = int(rs.randint(1, 40))
        Y = np.round(rs.rand(n, 2) * 1.3, 1 if case % 2 else 6)            # a coarse grid: duplicates and ties
        if case % 5 == 0:
            Y[rs.randint(n)] = REF                                          # a point ON the reference point
        front, idx = pareto_front_2d(Y, REF)
        assert list(idx) == _brute_front(Y, REF) and _bits(front, Y[idx].reshape(-1, 2)), case
        assert np.all(np.diff(front[:, 0]) > 0) and np.all(np.diff(front[:, 1]) < 0)
        # the area by brute force: per interval between two first objectives, the height the lowest point to its left leaves
        area = 0.0
        inside = Y[(Y[:, 0] < REF[0]) & (Y[:, 1] < REF[1])]
        xs = np.unique(np.concatenate((inside[:, 0], REF[:1])))
        for x0, x1 in zip(xs[:-1], xs[1:]):
            area += (x1 - x0) * (REF[1] - inside[inside[:, 0] <= x0, 1].min())
        assert abs(hypervolume_2d(front, REF) - area) <= 1e-13, case
        assert abs(exclusive_contributions_2d(front, REF).sum() - area) <= area + 1e-13
    front, idx = pareto_front_2d(np.array([[1.1, 0.2], [0.3, 1.1], [2.0, 2.0]]), REF)     # on and beyond ref: nothing left
    assert front.shape == (0, 2) and idx.shape == (0,) and hypervolume_2d(front, REF) == 0.0
    front, idx = pareto_front_2d(np.array([[0.5, 0.5], [0.5, 0.5], [0.2, 0.9], [0.5, 0.4]]), REF)
    assert list(idx) == [2, 3] and abs(hypervolume_2d(front, REF) - (0.9 * 0.2 + 0.6 * 0.5)) < 1e-15
    assert np.allclose(exclusive_contributions_2d(front, REF), [0.3 * 0.2, 0.6 * 0.5])


# ---- a. the moments form ---------------------------------------------------------------------------------------------------
def _group(P):
    """the issue's inputs for one P: 401 candidates, shared by every m"""
    rs = np.random.RandomState(100 + P)
    front = _curve_front(rs, P)
    mean = rs.rand(401, 2) * 1.1
    s = 0.055 + rs.rand(401, 2) * (1.1 - 0.055)
    return front, mean[:, 0].copy(), s[:, 0] ** 2, mean[:, 1].copy(), s[:, 1] ** 2


def _check_moments(ctx, label):
    worst = _Worst()
    for P in PS:
        front, mu1, v1, mu2, v2 = _group(P)
        orc = _oracle(("group", P), mu1, v1, mu2, v2, front, REF)
        assert np.mean(np.asarray(orc[0], dtype=np.float64) > TINY) >= 0.95, P
        full = None
        for m in MS[::-1]:
            vals, mx, am, fl = _lib.ehvi_from_moments(ctx, mu1[:m], v1[:m], mu2[:m], v2[:m], front, REF)
            _check_values(vals, [a[:m] for a in orc], "%s P = %d m = %d" % (label, P, m), worst)
            assert am == EO.np_argmax(vals) and _bits([mx], [vals[am]]) and fl == 0, (P, m)
            full = vals if full is None else full
            assert _bits(vals, full[:m]), (P, m)                   # a candidate's bits do not depend on m
    print("%s: moments groups, largest error / (eps unit) = %.3g" % (label, worst.ratio))
    assert worst.ratio <= EO.BOUND_FACTOR
    return worst.ratio


def _check_moments_special(ctx, label):
    worst = _Worst()
    rs = np.random.RandomState(5)
    front = _curve_front(rs, 9)

    def run(mu1, v1, mu2, v2, fr=front, ref=REF, tag="", flags=0):
        args = [np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (mu1, v1, mu2, v2)]
        vals, mx, am, fl = _lib.ehvi_from_moments(ctx, *args, fr, ref)
        _check_values(vals, _oracle(None, *args, fr, ref), "%s %s" % (label, tag), worst)
        assert fl == flags and am == EO.np_argmax(vals) and _bits([mx], [vals[am]]), (tag, fl)
        return vals
    m = 50
    mu1, mu2 = rs.rand(m) * 1.1, rs.rand(m) * 1.1
    v1, v2 = (0.055 + rs.rand(m)) ** 2, (0.055 + rs.rand(m)) ** 2
    zero = np.zeros(m)
    # zero sigma in either objective and in both: the max branch, flagged, not zeroed
    z1 = run(mu1, zero, mu2, v2, tag="s1 = 0", flags=_lib.FLAG_ZERO_SIGMA)
    z2 = run(mu1, v1, mu2, zero, tag="s2 = 0", flags=_lib.FLAG_ZERO_SIGMA)
    z12 = run(mu1, zero, mu2, zero, tag="s1 = s2 = 0", flags=_lib.FLAG_ZERO_SIGMA)
    gain = EO.hvi(mu1, mu2, front, REF)
    assert np.max(np.abs(z12 - gain)) <= 8 * EPS and gain.max() > 0.1 and z1.max() > 0 and z2.max() > 0
    one = run(np.where(np.arange(m) == 7, mu1, mu1), np.where(np.arange(m) == 7, 0.0, v1), mu2, v2, tag="one zero sigma",
              flags=_lib.FLAG_ZERO_SIGMA)
    assert _bits([one[7]], [z1[7]])
    # a mean more than 36 s above ref in either coordinate: exactly 0.0
    s = np.sqrt(v1)
    assert _bits(run(REF[0] + 36.001 * s, v1, mu2, v2, tag="36 s above ref, objective 1"), zero)
    assert _bits(run(mu1, v1, REF[1] + 36.001 * np.sqrt(v2), v2, tag="36 s above ref, objective 2"), zero)
    near = run(REF[0] + 35.0 * s, v1, mu2, v2, tag="35 s above ref")
    assert np.all(near > 0) and np.all(near < 1e-260)
    # far below the whole front: about the box down to the candidate, less what the front dominates already
    from robo_amd.util.pareto import hypervolume_2d
    far = run([-5.0, -50.0], [1e-4, 1.0], [-7.0, -20.0], [1e-4, 4.0], tag="far below the front")
    box = np.array([(REF[0] + 5.0) * (REF[1] + 7.0), (REF[0] + 50.0) * (REF[1] + 20.0)]) - hypervolume_2d(front, REF)
    assert np.max(np.abs(far / box - 1.0)) < 1e-12
    # sitting on a front point, on every one of them, with a small and a large sigma
    for sig in (1e-3, 0.3):
        on = run(front[:, 0], np.full(9, sig ** 2), front[:, 1], np.full(9, sig ** 2), tag="on a front point")
        assert np.all(on > 0)
    # P = 0: g(r1) g(r2)
    p0 = run(mu1, v1, mu2, v2, fr=np.zeros((0, 2)), tag="P = 0")
    G1, G2 = EO.g(REF[:1], mu1, np.sqrt(v1.astype(LD)))[0][:, 0], EO.g(REF[1:], mu2, np.sqrt(v2.astype(LD)))[0][:, 0]
    assert np.max(np.abs(p0 / np.asarray(G1 * G2, dtype=np.float64) - 1.0)) < 1e-13
    # a common scale: values scale with its square
    base = run(mu1, v1, mu2, v2, tag="scale 1")
    for sc in (1e-6, 1e6):
        scaled = run(mu1 * sc, v1 * sc * sc, mu2 * sc, v2 * sc * sc, fr=front * sc, ref=REF * sc, tag="scale %g" % sc)
        assert np.max(np.abs(scaled / (base * sc * sc) - 1.0)) < 1e-9
    # NaN in each of the four moments: NaN, the flag, argmax at the first NaN
    for k in range(4):
        args = [mu1.copy(), v1.copy(), mu2.copy(), v2.copy()]
        args[k][[30, 11]] = np.nan
        vals, mx, am, fl = _lib.ehvi_from_moments(ctx, *args, front, REF)
        assert np.isnan(vals[[11, 30]]).all() and np.isnan(vals).sum() == 2 and _bits(np.delete(vals, [11, 30]), np.delete(base, [11, 30]))
        assert fl == _lib.FLAG_NAN and np.isnan(mx) and am == 11, (k, am, fl)
    # duplicated candidates: the first index
    i = EO.np_argmax(base)
    j = 45 if i < 45 else 3
    args = [mu1.copy(), v1.copy(), mu2.copy(), v2.copy()]
    for a in args:
        a[j] = a[i]
    vals, mx, am, fl = _lib.ehvi_from_moments(ctx, *args, front, REF)
    assert vals[i] == vals[j] == mx and am == min(i, j)
    # the same rows inside two different batches, at other positions: the same bits; two calls: the same bits
    big = [np.concatenate((rs.rand(130), a[::-1], rs.rand(77) + 0.01)) for a in (mu1, v1, mu2, v2)]
    vals, _, _, _ = _lib.ehvi_from_moments(ctx, *big, front, REF)
    assert _bits(vals[130:130 + m][::-1], base)
    assert _bits(_lib.ehvi_from_moments(ctx, *big, front, REF)[0], vals)
    # argument errors: the status, and nothing launched (the library's last error names the reason)
    bad_fronts = [np.array([[0.2, 0.8], [0.2, 0.5]]),                      # a not strictly ascending
                  np.array([[0.2, 0.5], [0.4, 0.5]]),                      # b not strictly descending
                  np.array([[0.4, 0.5], [0.2, 0.8]]),                      # unsorted
                  np.array([[0.2, 1.1]]), np.array([[1.1, 0.2]]), np.array([[1.2, 0.2]]),      # not strictly below ref
                  np.array([[np.nan, 0.2]]), np.array([[0.2, np.inf]]), np.array([[-np.inf, 0.2]])]
    for fr in bad_fronts:
        with pytest.raises(ValueError):
            _lib.ehvi_from_moments(ctx, mu1, v1, mu2, v2, fr, REF)
    for ref in ([np.nan, 1.1], [1.1, np.inf]):
        with pytest.raises(ValueError):
            _lib.ehvi_from_moments(ctx, mu1, v1, mu2, v2, front, ref)
    ok_front = _curve_front(rs, _lib.EHVI_MAX_FRONT)
    assert np.all(np.isfinite(_lib.ehvi_from_moments(ctx, mu1[:3], v1[:3], mu2[:3], v2[:3], ok_front, REF)[0]))
    with pytest.raises(ValueError):
        _lib.ehvi_from_moments(ctx, mu1, v1, mu2, v2, _curve_front(rs, _lib.EHVI_MAX_FRONT + 1), REF)
    best, out = _lib._Best(), np.empty(m)
    fr = np.ascontiguousarray(front)
    args = [_lib._arr(mu1), _lib._arr(v1), _lib._arr(mu2), _lib._arr(v2), _lib._arr(fr), 9, _lib._arr(REF)]
    call = _lib.lib().robo_ehvi_eval_moments
    for k in (0, 1, 2, 3, 4, 6):
        a = list(args)
        a[k] = None
        assert call(ctx._h, m, *a, _lib._arr(out), *best.refs) == _lib.BAD_ARGUMENT, k
    a = list(args)
    a[5] = -1
    assert call(ctx._h, m, *a, _lib._arr(out), *best.refs) == _lib.BAD_ARGUMENT
    assert call(None, m, *args, _lib._arr(out), *best.refs) == _lib.BAD_ARGUMENT
    assert call(ctx._h, m, *args, _lib._arr(out), *best.refs) == _lib.OK and _bits(out, base)
    print("%s: chosen cases, largest error / (eps unit) = %.3g" % (label, worst.ratio))
    assert worst.ratio <= EO.BOUND_FACTOR
    return worst.ratio


# ---- b. the fused form -------------------------------------------------------------------------------------------------------
def _theta(D, ls2, noise=1e-2, amp=0.0):
    return np.concatenate([[amp], np.log(np.broadcast_to(ls2, (D,))), [np.log(noise)]])


def _data(N, D, seed):
    rs = np.random.RandomState(seed)
    X = rs.rand(N, D)
    y1 = np.sin(3 * X.sum(axis=1) / np.sqrt(D / 3.0)) + 0.1 * rs.randn(N)
    y2 = np.cos(2 * X[:, 0] - X[:, 1]) + 0.5 * (X[:, -1] - 0.3) ** 2 + 0.1 * rs.randn(N)
    return rs, X, y1, y2


def _fit(ctx, kind, theta, X, y):
    g = _lib.DeviceGP(ctx, kind, X.shape[0], X.shape[1])
    g.set_data(X, y)
    g.fit(theta, float(np.mean(y)))
    return g


def _pair(ctx, N, D, seed):
    from robo_amd.util.pareto import pareto_front_2d
    rs, X, y1, y2 = _data(N, D, seed)
    th1 = _theta(D, np.array([0.3, 0.5, 0.8, 0.4])[:D])
    th2 = _theta(D, np.array([0.9, 0.6, 0.4, 0.7])[:D], noise=3e-2, amp=0.3)
    g1, g2 = _fit(ctx, "matern52", th1, X, y1), _fit(ctx, "rbf", th2, X, y2)
    ref = np.array([y1.max() + 0.1, y2.max() + 0.1])
    front, _ = pareto_front_2d(np.stack((y1, y2), axis=1), ref)
    return rs, X, (y1, y2), (th1, th2), (g1, g2), front, ref


def _oracle_moments(key, X, ys, thetas, Xc):
    """oracle.gp_oracle's posterior of both objectives, variance floored as the device floors it; once per key"""
    if key not in _ORACLE:
        out = []
        for kind, th, y in zip(("matern52", "rbf"), thetas, ys):
            L = O.gp_compute(kind, th, X)
            mu, var = O.gp_predict_diag(kind, th, L, X, y, float(np.mean(y)), Xc)
            out += [mu, np.maximum(var, EPS)]
        _ORACLE[key] = out
    return _ORACLE[key]


def _check_fused_one(ctx, g1, g2, cand, front, ref, label, worst, rows=None, key=None):
    r = g1.ehvi(g2, cand, front, ref, diagnostics=True)
    assert r.trace.shape == (cand.m, 4) and r.flags == 0 and r.values.shape == (cand.m,), label
    # the trace is what robo_gp_predict_cand returns, bit for bit
    for o, g in enumerate((g1, g2)):
        mean, var = g.predict(cand)
        assert _bits(r.trace[:, 2 * o], mean) and _bits(r.trace[:, 2 * o + 1], var), (label, o)
    tr = r.trace if rows is None else r.trace[rows]
    orc = _oracle(key, tr[:, 0], tr[:, 1], tr[:, 2], tr[:, 3], front, ref)
    _check_values(r.values, orc, label, worst, rows)
    vals, mx, am, fl = _lib.ehvi_from_moments(ctx, *r.trace.T, front, ref)
    assert _bits(vals, r.values) and _bits([mx], [r.max]) and am == r.argmax and fl == r.flags, label
    assert r.argmax == EO.np_argmax(r.values) and _bits([r.max], [r.values[r.argmax]]), label
    r2 = g1.ehvi(g2, cand, front, ref, diagnostics=True)
    assert _bits(r2.values, r.values) and _bits(r2.trace, r.trace), label
    r3 = g1.ehvi(g2, cand, front, ref, want_values=False)
    assert r3.values is None and r3.trace is None and (r3.max, r3.argmax, r3.flags) == (r.max, r.argmax, r.flags), label
    return r


def _check_fused(ctx, label):
    worst = _Worst()
    sz = SMALL
    rs, X, ys, thetas, (g1, g2), front, ref = _pair(ctx, sz["N"], sz["D"], 0)
    assert front.shape[0] >= 3
    Xc_all = rs.rand(max(sz["Ms"]), sz["D"])
    other = _lib.Context(0)
    try:
        for M in sz["Ms"]:
            cand = _lib.Candidates(ctx, Xc_all[:M])
            fresh = _lib.Candidates(ctx, Xc_all[:M])
            try:
                tag = "%s M = %d" % (label, M)
                # EI of gp1 on a handle no EHVI call has touched, and on this one before and after
                ei_fresh = g1.acq("ei", 0.0, float(ys[0].min()), fresh)
                ei_before = g1.acq("ei", 0.0, float(ys[0].min()), cand)
                r = _check_fused_one(ctx, g1, g2, cand, front, ref, tag, worst, key=("fused", label, M))
                ei_after = g1.acq("ei", 0.0, float(ys[0].min()), cand)
                for a, b, c in zip(ei_fresh, ei_before, ei_after):
                    assert _bits([a], [b]) and _bits([a], [c]), tag
                # against the fp64 oracle's posterior
                om = _oracle_moments("small", X, ys, thetas, Xc_all)
                want = np.asarray(EO.ehvi_batch(*[a[:M] for a in om], front, ref)[0], dtype=np.float64)
                print("%s: against gp_oracle's posterior, worst relative difference %.3e"
                      % (tag, np.max(np.abs(r.values - want) / want)))
                np.testing.assert_allclose(r.values, want, rtol=ACQ_RTOL, atol=0, err_msg=tag)
                # several passes through a small workspace: the same bits
                n_pad = 128
                ctx.set_tuning("ws_bytes", 128 * n_pad * 8)
                try:
                    rp = g1.ehvi(g2, cand, front, ref, diagnostics=True)
                    assert cand.chunk() == 128 and M > 3 * 128
                finally:
                    ctx.set_tuning("ws_bytes", None)
                assert _bits(rp.values, r.values) and _bits(rp.trace, r.trace) and rp.argmax == r.argmax, tag
                # an empty front
                r0 = g1.ehvi(g2, cand, np.zeros((0, 2)), ref, diagnostics=True)
                _check_values(r0.values, _oracle(None, *r0.trace.T, np.zeros((0, 2)), ref), tag + " P = 0", worst)
            finally:
                cand.close()
                fresh.close()
        # refusals: nothing is launched, the handles stay usable
        cand = _lib.Candidates(ctx, Xc_all[:64])
        wide = _lib.Candidates(ctx, rs.rand(5, sz["D"] + 1))
        far = _lib.Candidates(other, Xc_all[:5])
        g_far = _fit(other, "rbf", thetas[1], X, ys[1])
        raw = _lib.DeviceGP(ctx, "matern52", sz["N"], sz["D"])
        try:
            with pytest.raises(ValueError):
                g1.ehvi(g_far, cand, front, ref)                               # GPs on different contexts
            with pytest.raises(ValueError):
                g1.ehvi(g2, far, front, ref)                                   # the candidates on another context
            with pytest.raises(_lib.RoboBadShape):
                g1.ehvi(g2, wide, front, ref)
            for a, b in ((raw, g2), (g1, raw)):
                with pytest.raises(Exception, match="trained first"):
                    a.ehvi(b, cand, front, ref)
            with pytest.raises(ValueError):
                g1.ehvi(g2, cand, front[::-1], ref)
            with pytest.raises(ValueError):
                g1.ehvi(g2, cand, front, ref - 10.0)
            best = _lib._Best()
            call = _lib.lib().robo_ehvi_eval_cand
            fr = np.ascontiguousarray(front)
            for a in ((None, g2._h, cand._h), (g1._h, None, cand._h), (g1._h, g2._h, None)):
                assert call(*a, _lib._arr(fr), fr.shape[0], _lib._arr(ref), None, *best.refs, None) == _lib.BAD_ARGUMENT
            assert call(g1._h, g2._h, cand._h, _lib._arr(fr), fr.shape[0], None, None, *best.refs, None) == _lib.BAD_ARGUMENT
            ok = g1.ehvi(g2, cand, front, ref)
            assert ok.flags == 0 and np.all(np.isfinite(ok.values)) and np.all(ok.values >= 0)
        finally:
            for h in (cand, wide, far, g_far, raw):
                h.close()
    finally:
        other.close()
        g1.close()
        g2.close()
    print("%s: fused cases, largest error / (eps unit) = %.3g" % (label, worst.ratio))
    assert worst.ratio <= EO.BOUND_FACTOR
    return worst.ratio


# ---- c. host classes and the front end ---------------------------------------------------------------------------------------
_BOX = (np.zeros(2), np.ones(2))
_TOY_REF = np.array([2.5, 2.5])


def _toy(x):
    x = np.asarray(x, dtype=np.float64)
    return float(np.sum(x ** 2)), float(np.sum((x - 1.0) ** 2))


def _gp_models(n=12, seed=0):
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models import GaussianProcess
    rs = np.random.RandomState(seed)
    X = rs.rand(n, 2)
    Y = np.array([_toy(x) for x in X])
    models = []
    for o, ls in enumerate((0.6, 0.9)):
        m = GaussianProcess(Matern52Kernel(np.array([ls, ls]), ndim=2), noise=1e-3, lower=_BOX[0], upper=_BOX[1],
                            normalize_output=bool(o))
        m.train(X, Y[:, o].copy(), do_optimize=False)
        models.append(m)
    return rs, X, Y, models


class _Foreign(object):
    """not a device model for the class: predict() and the training data of a wrapped GP alone (the moments path)"""

    def __init__(self, model, Y):
        self._m, self.X, self.y = model, model.X, Y
        self.lower, self.upper = model.lower, model.upper

    normalize_input = property(lambda self: self._m.normalize_input)

    def predict(self, X):
        return self._m.predict(X)


def _check_class(ctx):
    from robo_amd.acquisition_functions import EHVI
    from robo_amd.maximizers import RandomSampling
    from robo_amd.maximizers.random_sampling import DeviceRandomSampling
    from robo_amd.util.pareto import exclusive_contributions_2d, pareto_front_2d
    worst = _Worst()
    rs, X, Y, models = _gp_models()
    acq = EHVI(models, _TOY_REF)
    acq.update(models)
    front, idx = pareto_front_2d(Y, _TOY_REF)
    # (objective 2 is normalised inside its model: its targets come back through y * y_std + y_mean)
    assert np.allclose(acq.front, front, rtol=1e-14, atol=0) and front.shape[0] >= 2
    assert not hasattr(acq.model, "models") and acq.model.objectives == models
    Xc = rs.rand(70, 2)
    a = acq.compute(Xc)
    assert a.shape == (70,) and np.all(a >= 0) and np.all(np.isfinite(a)) and _bits(acq.compute(Xc), a)
    i = acq.argmax(Xc)
    assert i == EO.np_argmax(a) == acq.last_argmax and _bits([acq.last_max], [a[i]])
    # the native path against the moments path on the same models, within the value bound
    foreign = EHVI([_Foreign(models[0], Y[:, 0]), _Foreign(models[1], Y[:, 1])], _TOY_REF)
    assert not foreign._is_native() and acq._is_native() and _bits(foreign.front, front)
    mom = foreign.moments(Xc)
    b = foreign.compute(Xc)
    orc = _oracle(None, *mom, front, _TOY_REF)
    _check_values(b, orc, "class, moments path", worst)
    _check_values(a, _oracle(None, *mom, acq.front, _TOY_REF), "class, native path", worst)
    assert foreign.argmax(Xc) == EO.np_argmax(b) == foreign.last_argmax
    # a device batch in the normalised box is the same call
    cand = _lib.Candidates(models[0].gp.ctx, models[0]._normalised(Xc))
    try:
        assert _bits(acq.compute(cand), a) and acq.argmax(cand) == i and _bits(foreign.compute(cand), b)
        models[0].normalize_input = False
        try:
            with pytest.raises(TypeError):
                foreign.compute(cand)
        finally:
            models[0].normalize_input = True
    finally:
        cand.close()
    # the incumbent: the front point with the largest exclusive contribution; with an empty front the lowest first objective
    x_inc, y_inc = acq.model.get_incumbent()
    j = idx[np.argmax(exclusive_contributions_2d(front, _TOY_REF))]
    assert np.allclose(x_inc, X[j], rtol=0, atol=1e-15) and np.allclose(y_inc, Y[j], rtol=1e-14, atol=0)
    empty = EHVI(models, [-1.0, -1.0])
    assert empty.front.shape == (0, 2) and np.allclose(empty.model.get_incumbent()[1], Y[np.argmin(Y[:, 0])], rtol=1e-14)
    e = empty.compute(Xc[:5])
    _check_values(e, _oracle(None, *[m[:5] for m in mom], np.zeros((0, 2)), [-1.0, -1.0]), "class, empty front", worst)
    # deepcopy evaluates to the same bits; update() takes a new pair
    dup = copy.deepcopy(acq)
    assert dup.model is not acq.model and _bits(dup.compute(Xc), a) and _bits(dup.front, acq.front)
    # the maximisers that draw around the incumbent
    np.random.seed(4)
    for mk in (lambda: RandomSampling(acq, _BOX[0], _BOX[1], n_samples=60),
               lambda: DeviceRandomSampling(acq, _BOX[0], _BOX[1], n_samples=128, rng=np.random.RandomState(9))):
        x = mk().maximize()
        assert x.shape == (2,) and np.all(x >= _BOX[0]) and np.all(x <= _BOX[1])
    # refusals
    with pytest.raises(NotImplementedError):
        acq.compute(Xc, derivative=True)
    with pytest.raises(NotImplementedError):
        acq.argmax_sharded(None, Xc[:10], 0)
    with pytest.raises(NotImplementedError):
        RandomSampling(acq, _BOX[0], _BOX[1], n_samples=60, shard=True).maximize()
    models[1].devices = [0, 1]
    try:
        for call in (lambda: acq.argmax(Xc), lambda: acq.compute(Xc)):
            with pytest.raises(NotImplementedError, match="devices"):
                call()
    finally:
        models[1].devices = None
    with pytest.raises(ValueError):
        EHVI(models[:1], _TOY_REF)
    with pytest.raises(ValueError):
        EHVI(models, [np.nan, 1.0])
    short = _Foreign(models[1], Y[:-1, 1])
    with pytest.raises(ValueError):
        EHVI([models[0], short], _TOY_REF)
    assert worst.ratio <= EO.BOUND_FACTOR


def _check_class_mcmc(ctx):
    from robo_amd.acquisition_functions import EHVI
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models.gaussian_process_mcmc import GaussianProcessMCMC
    from robo_amd.priors.default_priors import DefaultPrior
    from robo_amd.util.pareto import pareto_front_2d
    worst = _Worst()
    rs = np.random.RandomState(2)
    X = rs.rand(10, 2)
    Y = np.array([_toy(x) for x in X])
    models = []
    for o in range(2):
        kernel = 2 * Matern52Kernel(np.ones(2), ndim=2)
        m = GaussianProcessMCMC(kernel, prior=DefaultPrior(len(kernel) + 1, rng=np.random.RandomState(3 + o)), n_hypers=8,
                                chain_length=4, burnin_steps=2, rng=np.random.RandomState(4 + o), lower=_BOX[0],
                                upper=_BOX[1])
        m.train(X, Y[:, o].copy())
        models.append(m)
    acq = EHVI(models, _TOY_REF)
    assert not acq._is_native() and _bits(acq.front, pareto_front_2d(Y, _TOY_REF)[0])
    Xc = rs.rand(40, 2)
    a = acq.compute(Xc)
    mom = [np.asarray(v, dtype=np.float64).ravel() for m in models for v in m.predict(Xc)]       # the mixture moments
    _check_values(a, _oracle(None, *mom, acq.front, _TOY_REF), "class, gp_mcmc pair", worst)
    assert acq.argmax(Xc) == EO.np_argmax(a) and np.all(a >= 0) and a.max() > 0
    assert worst.ratio <= EO.BOUND_FACTOR


def _random_search_hv(n, seed):
    """the hypervolume of n uniform points drawn as fmin/random_search.py draws them (rng.uniform(lower, upper) per point)"""
    from robo_amd.util.pareto import hypervolume_2d, pareto_front_2d
    rng = np.random.RandomState(seed)
    Y = np.array([_toy(rng.uniform(_BOX[0], _BOX[1])) for _ in range(n)])
    return hypervolume_2d(pareto_front_2d(Y, _TOY_REF)[0], _TOY_REF)


def _check_front_end(ctx):
    """f1 = |x|^2, f2 = |x - 1|^2 on [0, 1]^2, ref (2.5, 2.5), 3 initial points + 5 iterations, 128 candidates, seed 1.  Final
    hypervolume through the interpreter: "random" 5.1848, "device_random" 5.1845; a random_search-style run of 8 evaluations
    on the same seed: 4.7761.  (Seeds 0 .. 9, interpreter: 19 of the 20 runs end above their random search -- by 0.02 to
    0.41 --, seed 8 with "device_random" ends 0.07 below a random search that drew 5.21.)"""
    from robo_amd.fmin import multi_objective_optimization
    from robo_amd.util.pareto import hypervolume_2d, pareto_front_2d
    baseline = _random_search_hv(8, 1)
    for maximizer in ("random", "device_random"):
        np.random.seed(1)
        calls = []

        def f(x):
            calls.append(np.array(x))
            return _toy(x)
        res = multi_objective_optimization(f, _BOX[0], _BOX[1], _TOY_REF, num_iterations=8, n_init=3, maximizer=maximizer,
                                           model_type="gp", n_candidates=128, rng=np.random.RandomState(1))
        X, Y, hv = np.array(res["X"]), np.array(res["Y"]), np.array(res["hypervolume"])
        assert X.shape == (8, 2) and Y.shape == (8, 2) and len(calls) == 8 and hv.shape == (8,)
        assert np.all(X >= _BOX[0]) and np.all(X <= _BOX[1]) and np.all(np.isfinite(Y))
        assert np.all(np.diff(hv) >= 0), hv
        front, idx = pareto_front_2d(Y, _TOY_REF)
        assert _bits(res["pareto_Y"], front) and _bits(res["pareto_X"], X[idx])
        assert hv[-1] == hypervolume_2d(front, _TOY_REF)
        assert len(res["runtime"]) == 8 and len(res["overhead"]) == 8
        print("multi_objective_optimization(%s): final hypervolume %.4f, random search %.4f" % (maximizer, hv[-1], baseline))
        assert hv[-1] >= baseline, (maximizer, hv[-1], baseline)
    with pytest.raises(ValueError):
        multi_objective_optimization(_toy, _BOX[0], _BOX[1], _TOY_REF, maximizer="scipy")
    with pytest.raises(ValueError):
        multi_objective_optimization(_toy, _BOX[0], _BOX[1], _TOY_REF, model_type="rf")
    with pytest.raises(ValueError):
        multi_objective_optimization(_toy, _BOX[0], _BOX[1], _TOY_REF, model_type="gp_mcmc", maximizer="device_random")


def _check_front_end_mcmc(ctx):
    from robo_amd.fmin import multi_objective_optimization
    np.random.seed(5)
    res = multi_objective_optimization(_toy, _BOX[0], _BOX[1], _TOY_REF, num_iterations=4, n_init=3, model_type="gp_mcmc",
                                       n_candidates=60, rng=np.random.RandomState(5), chain_length=4, burnin_steps=2)
    hv = np.array(res["hypervolume"])
    assert hv.shape == (4,) and np.all(np.diff(hv) >= 0) and np.array(res["Y"]).shape == (4, 2)


# ---- the runs ------------------------------------------------------------------------------------------------------------------
def test_moments_emu(emu_ctx):
    _check_moments(emu_ctx, "interpreter")
    _check_moments_special(emu_ctx, "interpreter")


def test_fused_emu(emu_ctx):
    _check_fused(emu_ctx, "interpreter")


def test_classes_emu(emu_ctx):
    _check_class(emu_ctx)
    _check_class_mcmc(emu_ctx)


def test_front_end_emu(emu_ctx):
    _check_front_end(emu_ctx)
    _check_front_end_mcmc(emu_ctx)


@pytest.mark.parametrize("model_type", ["gp", "gp_mcmc"])
def test_front_end_trajectory_emu(emu_ctx, model_type):
    """a seeded run on the interpreter repeats, bit for bit, the trajectory recorded before the front ends' shared loop was
    stated once (tests/golden/fmin_trajectories.json; NOTES.md names the commit): the points ``rng`` is consumed at, and
    every number behind the proposals, are where they were"""
    import json
    from robo_amd.fmin import multi_objective_optimization
    with open(os.path.join(HERE, "golden", "fmin_trajectories.json")) as f:
        want = json.load(f)["multi_objective/" + model_type]
    kw = dict(chain_length=4, burnin_steps=2) if model_type == "gp_mcmc" else {}
    np.random.seed(11)
    res = multi_objective_optimization(_toy, _BOX[0], _BOX[1], _TOY_REF, num_iterations=5, n_init=3, n_candidates=32,
                                       model_type=model_type, rng=np.random.RandomState(11), **kw)
    assert np.array(res["X"]).shape == (5, 2)
    for key in ("X", "Y"):
        assert _bits(res[key], want[key]), (key, res[key], want[key])


@pytest.mark.gpu
def test_moments_gpu(gpu_ctx):
    _check_moments(gpu_ctx, "MI355X")
    _check_moments_special(gpu_ctx, "MI355X")


@pytest.mark.gpu
def test_fused_gpu(gpu_ctx):
    _check_fused(gpu_ctx, "MI355X")


@pytest.mark.gpu
def test_classes_and_front_end_gpu(gpu_ctx):
    _check_class(gpu_ctx)
    _check_class_mcmc(gpu_ctx)
    _check_front_end(gpu_ctx)
    _check_front_end_mcmc(gpu_ctx)


@pytest.mark.gpu
def test_fused_large_gpu(gpu_ctx):
    """N = 256, D = 4, m = 32 773, P = 50 (a curve front across the targets' range): every 97th candidate and the last six"""
    sz = LARGE
    worst = _Worst()
    rs, X, ys, thetas, (g1, g2), _, ref = _pair(gpu_ctx, sz["N"], sz["D"], 4)
    lo = np.array([ys[0].min(), ys[1].min()])
    front = lo + _curve_front(rs, sz["P"]) * (ref - 0.05 - lo)
    Xc = rs.rand(sz["M"], sz["D"])
    cand = _lib.Candidates(gpu_ctx, Xc)
    try:
        rows = np.concatenate((np.arange(0, sz["M"], 97), np.arange(sz["M"] - 6, sz["M"])))
        r = _check_fused_one(gpu_ctx, g1, g2, cand, front, ref, "fused large", worst, rows)
        om = _oracle_moments("large", X, ys, thetas, Xc[rows])
        want = np.asarray(EO.ehvi_batch(*om, front, ref)[0], dtype=np.float64)
        np.testing.assert_allclose(r.values[rows], want, rtol=ACQ_RTOL, atol=0)
        # (256 observations leave a tight posterior: a third of these candidates sit many sigmas above the front and are
        # worth 1e-20 and less -- still compared to 1e-7 relative above; the case is not degenerate while they are non-zero
        # and the best ones are a sizeable part of the box)
        assert np.mean(want > 0) >= 0.95 and want.max() > 1e-3 * float(np.prod(ref - lo))
        print("MI355X: fused large, largest error / (eps unit) = %.3g" % worst.ratio)
        assert worst.ratio <= EO.BOUND_FACTOR
    finally:
        cand.close()
        g1.close()
        g2.close()
