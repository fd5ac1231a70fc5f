"""Constrained expected improvement (robo_amd/csrc/cei.hip, api_cei.hip: robo_cei_eval_cand, robo_cei_eval_moments; the
ConstrainedEI class and the constrained_optimization front end) against tests/cei_oracle.py.

CPU: through the interpreter (tests/hipemu).  -m gpu: the same checks at the same small shapes on the MI355X, plus the fused
form at N = 256, D = 4, C = 2, m = 32 773.

The oracle is the rule in np.longdouble fed THE DEVICE'S OWN DOUBLES (the trace, or the inputs of the moments form), itself
checked against a trapezoid quadrature of E[(eta - y)^+ prod_k 1[c_k <= t_k]] (test_oracle).  The bound, per candidate and
per mode, is derived in tests/cei_oracle.py from the conditioning of each factor; it is not tuned.  Three kinds of check:

    PoF / L alone (eta None)   the constraints' side only: 2 eps unit_L [+ exp's rounding]
    fold                       the value against the oracle's L and the objective factor of the device's own trace
    total                      the value against the oracle's own objective factor, which carries what the EI tests grant it

The fused cases keep the incumbent at the targets' upper quartile: EI's plain form z Phi + phi loses about z^4 eps to
cancellation, so its share of the total bound (the EI tests' 1e-10) is only meaningful for z_0 above about -12; the tails
(z down to -40) are exercised on the constraints' side.

Largest observed error / bound (the bound is the unit times the doubled count, so <= 1 passes), alone / fold / total:
    interpreter:   0.35 / - / 0.28 (moments groups), 0.084 / - / 6.6e-5 (chosen cases), 0.15 / 0.15 / 0.062 (fused cases),
                   0.11 / - / 0.059 (classes)
    MI355X:        0.35 / - / 0.28 (moments groups), 0.084 / - / 7.0e-5 (chosen cases), 0.15 / 0.15 / 0.067 (fused cases),
                   0.12 / - / 0.074 (classes), 0.13 / 0.13 / 0.048 (fused large)
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
import cei_oracle as CO  # noqa: E402

LD = CO.LD
CS = (0, 1, 2, 3, 16)
MS = (1, 63, 64, 65, 400, 401)
MODES = (("ei", 0.45), ("log_ei", 0.45), ("ei", None), ("log_ei", None))
PAR = 0.01
SMALL = dict(N=80, D=3, Ms=(400, 401))
LARGE = dict(N=256, D=4, M=32768 + 5)


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
    def __init__(self):
        self.ratio = {"alone": 0.0, "fold": 0.0, "total": 0.0}

    def take(self, kind, dev, orc, label):
        r = CO.check(dev, orc)
        self.ratio[kind] = max(self.ratio[kind], r)
        assert r <= 1.0, (label, kind, r)

    def report(self, label):
        print("%s: largest error / bound: PoF or L alone %.3g, fold %.3g, total %.3g"
              % (label, self.ratio["alone"], self.ratio["fold"], self.ratio["total"]))


_ORACLE = {}


def _oracle(key, *args, **kw):
    """cei_batch on these doubles, computed once per key and shared between the interpreter and the MI355X runs"""
    if key is None:
        return CO.cei_batch(*args, **kw)
    stamp = b"".join(np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in args[:5])
    if key not in _ORACLE:
        out = CO.cei_batch(*args, **kw)
        for a in out.values():
            a.setflags(write=False)
        _ORACLE[key] = (out, stamp)
    out, have = _ORACLE[key]
    assert have == stamp, key
    return out


# ---- the oracle itself ----------------------------------------------------------------------------------------------------------
def test_oracle():
    """the rule in np.longdouble against the product trapezoid rule (200001 nodes per axis on +-9 s) of
    E[(eta - y)^+ prod_k 1[c_k <= t_k]]; log Phi against scipy where scipy is accurate; the pieces the bound uses"""
    from scipy.special import log_ndtr
    rs = np.random.RandomState(1)
    worst = 0.0
    for Cn in (0, 1, 2, 3):
        for _ in range(3):
            mu0, s0, eta = rs.rand(), 0.1 + rs.rand(), rs.rand()
            means, s, th = rs.randn(Cn), 0.1 + rs.rand(Cn), rs.randn(Cn) * 0.5
            val = float(CO.cei_batch([mu0], [s0 ** 2], means[:, None], (s ** 2)[:, None], th, "ei", 0.0, eta)["value"][0])
            q, factors, h = CO.quadrature(mu0, s0 ** 2, means, s ** 2, th, eta)
            tol = 1e-6 + sum(0.4 * h / f for f in factors)
            worst = max(worst, abs(val - q) / val)
            assert abs(val - q) <= tol * val, (Cn, val, q, tol)
            lval = float(CO.cei_batch([mu0], [s0 ** 2], means[:, None], (s ** 2)[:, None], th, "log_ei", 0.0, eta)["value"][0])
            assert abs(lval - np.log(val)) <= 1e-15 * (1 + abs(lval))
    print("oracle against quadrature: worst relative difference %.3e" % worst)
    z = np.concatenate((np.linspace(-40, 40, 161), [-1.0, -1.0 - 1e-9, -np.sqrt(2), 0.0]))
    l, odds, mills = CO.norm_cdf_pair(z)
    assert np.max(np.abs(np.asarray(l, dtype=np.float64) - log_ndtr(z)) / np.maximum(np.abs(log_ndtr(z)), 1e-300)) < 1e-12
    # Phi(-z) / Phi(z) and phi / Phi as the bound uses them: |z| phi / Phi <= z^2 + 1 on the left, <= 0.3 on the right
    amp = np.abs(z) * np.asarray(mills, dtype=np.float64)
    assert np.all(amp[z < 0] <= z[z < 0] ** 2 + 1) and np.all(amp[z >= 0] <= 0.3)
    assert abs(float(odds[-1]) - 1.0) < 1e-18 and abs(float(mills[-1]) - 2 / np.sqrt(2 * np.pi)) < 1e-16


def test_incumbent_rules():
    """the feasible incumbent: none feasible, one feasible, a tie on the objective, a violation exactly on the threshold"""
    from robo_amd.acquisition_functions.constrained_ei import feasible_incumbent, feasible_mask, least_violation
    th = np.array([0.0, 1.0])
    y = np.array([3.0, 1.0, 2.0, 1.0])
    none = np.array([[0.1, 0.0], [0.5, 2.0], [1e-300, 0.0], [0.0, 1.5]])
    assert feasible_incumbent(y, none, th) is None and not feasible_mask(none, th).any()
    assert least_violation(none, th) == 2                      # the smallest LARGEST violation
    one = none.copy()
    one[0] = [-0.1, 0.9]
    assert feasible_incumbent(y, one, th) == 0 and list(feasible_mask(one, th)) == [True, False, False, False]
    tie = np.array([[-1.0, 0.0], [-1.0, 0.0], [-1.0, 0.0], [-1.0, 0.0]])
    assert feasible_incumbent(y, tie, th) == 1                 # y[1] == y[3]: the lowest index
    on = none.copy()
    on[3] = [0.0, 1.0]                                         # exactly on both thresholds: feasible
    assert feasible_incumbent(y, on, th) == 3 and feasible_mask(on, th)[3]
    assert feasible_incumbent(y, np.zeros((4, 0)), np.zeros(0)) == 1          # no constraints: the plain incumbent


# ---- a. the moments form --------------------------------------------------------------------------------------------------------
def _group(Cn):
    """401 candidates for one C: objective z_0 within +-8 of eta, constraints' z spanning -40 .. 40 (every second candidate
    kept on the feasible side of -3, so that the weighted values are not all 0)"""
    rs = np.random.RandomState(200 + Cn)
    m = 401
    mu0, s0 = rs.rand(m), 0.07 + rs.rand(m)
    th = np.round(rs.randn(Cn), 2)
    z = np.array([rs.permutation(np.linspace(-40.0, 40.0, m)) for _ in range(Cn)]).reshape(Cn, m)
    z[:, ::2] = np.maximum(z[:, ::2], -3.0 * rs.rand(Cn, (m + 1) // 2))
    s = 0.05 + 2 * rs.rand(Cn, m)
    means = th[:, None] - z * s
    return mu0, s0 ** 2, means, s ** 2, th


def _check_moments(ctx, label):
    worst = _Worst()
    for Cn in CS:
        mu0, v0, means, vars_, th = _group(Cn)
        for kind, eta in MODES:
            orc = _oracle(("group", Cn, kind, eta), mu0, v0, means, vars_, th, kind=kind, par=PAR, eta=eta)
            full = None
            for m in MS[::-1]:
                tag = "%s C = %d %s eta %s m = %d" % (label, Cn, kind, eta, m)
                vals, mx, am, fl = _lib.cei_from_moments(ctx, mu0[:m], v0[:m], means[:, :m], vars_[:, :m], th, kind, PAR, eta)
                worst.take("alone" if eta is None else "total", vals, {k: a[:m] for k, a in orc.items()}, tag)
                assert am == CO.np_argmax(vals) and _bits([mx], [vals[am]]) and fl == 0, tag
                full = vals if full is None else full
                assert _bits(vals, full[:m]), tag                  # a candidate's bits do not depend on m
            if Cn and kind == "ei":
                # the left tail: the product reaches exactly 0 where the sum of logs is still finite
                logs = _lib.cei_from_moments(ctx, mu0, v0, means, vars_, th, "log_ei", PAR, eta)[0]
                assert np.any(full == 0.0) and np.all(np.isfinite(logs)) and np.any(full > 0.0), (Cn, eta)
                assert logs[full == 0.0].max() < -700
        if Cn == 0:
            # C = 0: robo_acq_eval_moments' bits, and the neutral elements without an incumbent
            for kind in ("ei", "log_ei"):
                want = _lib.acq_from_moments(ctx, kind, PAR, 0.45, mu0, v0)
                got = _lib.cei_from_moments(ctx, mu0, v0, means, vars_, th, kind, PAR, 0.45)
                assert _bits(got[0], want[0]) and got[1:] == want[1:], kind
            assert _bits(_lib.cei_from_moments(ctx, mu0, v0, means, vars_, th, "ei", 0.0, None)[0], np.ones(401))
            assert _bits(_lib.cei_from_moments(ctx, mu0, v0, means, vars_, th, "log_ei", 0.0, None)[0], np.zeros(401))
    worst.report(label + ", moments groups")
    return worst


def _check_moments_special(ctx, label):
    worst = _Worst()
    rs = np.random.RandomState(7)
    m, Cn = 70, 2
    mu0, v0 = rs.rand(m), (0.07 + rs.rand(m)) ** 2
    th = np.array([0.25, -0.5])
    s = 0.1 + rs.rand(Cn, m)
    means, vars_ = th[:, None] - rs.uniform(-2, 3, (Cn, m)) * s, s ** 2
    ZS, NEG, NAN = _lib.FLAG_ZERO_SIGMA, _lib.FLAG_NEGATIVE_EI, _lib.FLAG_NAN

    def run(kind, eta, mu0=mu0, v0=v0, means=means, vars_=vars_, th=th, tag="", flags=0):
        vals, mx, am, fl = _lib.cei_from_moments(ctx, mu0, v0, means, vars_, th, kind, PAR, eta)
        orc = CO.cei_batch(mu0, v0, means, vars_, th, kind, PAR, eta)
        worst.take("alone" if eta is None else "total", vals, orc, "%s %s %s %s" % (label, tag, kind, eta))
        assert fl == flags and am == CO.np_argmax(vals) and (_bits([mx], [vals[am]]) or np.isnan(mx)), (tag, kind, eta, fl)
        return vals
    base = {mode: run(*mode, tag="base") for mode in MODES}
    # zero sigma on the feasible side, exactly on the threshold and beyond it: factor 1, 1, 0, the flag
    for mode in MODES:
        kind, eta = mode
        for where, mu_k in (("below", th[1] - 0.3), ("on", th[1]), ("above", th[1] + 1e-12)):
            mk, vk = means.copy(), vars_.copy()
            mk[1, 10:20], vk[1, 10:20] = mu_k, 0.0
            vals = run(kind, eta, means=mk, vars_=vk, tag="zero sigma " + where, flags=ZS)
            assert _bits(np.delete(vals, range(10, 20)), np.delete(base[mode], range(10, 20)))
            # ... equal to the value without that constraint, or to the empty product
            one = _lib.cei_from_moments(ctx, mu0[10:20], v0[10:20], means[:1, 10:20], vars_[:1, 10:20], th[:1], kind, PAR, eta)[0]
            if where == "above":
                assert _bits(vals[10:20], np.full(10, -np.inf if kind == "log_ei" else 0.0)), mode
            else:
                assert _bits(vals[10:20], one), (mode, where)
    # s_0 == 0: the objective functions' own branches, the same flag (EI's plain form is 0 * inf there: NaN)
    v00 = v0.copy()
    v00[5] = 0.0
    vals = run("log_ei", 0.45, v0=v00, tag="s_0 = 0", flags=ZS)
    assert np.isfinite(vals[5]) == (mu0[5] < 0.45 - PAR)
    vals = run("ei", 0.45, v0=v00, tag="s_0 = 0", flags=ZS | NAN)
    assert np.isnan(vals[5]) and np.isnan(vals).sum() == 1
    assert run("ei", None, v0=v00, tag="s_0 = 0, no incumbent")[5] == base[("ei", None)][5]
    # a negative EI (the plain form's rounding far on the left, above DBL_MIN in size) keeps its flag
    far = _lib.acq_from_moments(ctx, "ei", 0.0, 0.0, np.linspace(20.0, 37.0, 400), np.ones(400))
    if far[3] & NEG:
        got = _lib.cei_from_moments(ctx, np.linspace(20.0, 37.0, 400), np.ones(400), np.zeros((1, 400)), np.ones((1, 400)),
                                    [5.0], "ei", 0.0, 0.0)
        assert got[3] & NEG
    # NaN in every moment, and a negative variance: NaN, the flag, argmax at the first NaN
    for mode in MODES:
        for which in range(6):
            args = [mu0.copy(), v0.copy(), means.copy(), vars_.copy()]
            tgt = args[which] if which < 2 else args[2 + (which - 2) % 2][(which - 2) // 2]
            tgt[[40, 13]] = np.nan if which != 5 else -1e-3
            vals, mx, am, fl = _lib.cei_from_moments(ctx, *args, th, mode[0], PAR, mode[1])
            assert np.isnan(vals[[13, 40]]).all() and np.isnan(vals).sum() == 2, (mode, which)
            assert _bits(np.delete(vals, [13, 40]), np.delete(base[mode], [13, 40]))
            assert fl == NAN and np.isnan(mx) and am == 13, (mode, which, am, fl)
            assert CO.check(vals, CO.cei_batch(*args, th, mode[0], PAR, mode[1])) <= 1.0
        v_neg = v0.copy()
        v_neg[3] = -1.0
        vals, mx, am, fl = _lib.cei_from_moments(ctx, mu0, v_neg, means, vars_, th, mode[0], PAR, mode[1])
        assert np.isnan(vals[3]) and am == 3 and fl == NAN, mode
    # ties: a duplicated best candidate wins at its first index; a planted maximum is found at every batch position
    for mode in MODES:
        i = CO.np_argmax(base[mode])
        for j in (0, 63, 64, m - 1):
            if j == i:
                continue
            args = [mu0.copy(), v0.copy(), means.copy(), vars_.copy()]
            for a in args:
                a[..., j] = a[..., i]
            vals, mx, am, _ = _lib.cei_from_moments(ctx, *args, th, mode[0], PAR, mode[1])
            assert vals[i] == vals[j] == mx and am == min(i, j), (mode, j)
            # the planted maximum: certainly feasible, far below the incumbent
            args = [mu0.copy(), v0.copy(), means.copy(), vars_.copy()]
            args[0][j], args[2][:, j] = -3.0, th - 50.0
            vals, mx, am, _ = _lib.cei_from_moments(ctx, *args, th, mode[0], PAR, mode[1])
            if mode[1] is not None:
                assert am == j and mx == vals[j], (mode, j)
            else:
                assert vals[j] == (1.0 if mode[0] == "ei" else 0.0) == mx and am == CO.np_argmax(vals), (mode, j)
    # the same rows inside another batch, at other positions: the same bits; two calls: the same bits
    for mode in MODES:
        pad = lambda a, lo, hi: np.concatenate((lo, a[..., ::-1], hi), axis=-1)                    # noqa: E731
        big = [pad(mu0, rs.rand(130), rs.rand(77)), pad(v0, rs.rand(130) + 0.01, rs.rand(77) + 0.01),
               pad(means, rs.randn(Cn, 130), rs.randn(Cn, 77)), pad(vars_, rs.rand(Cn, 130) + 0.01, rs.rand(Cn, 77) + 0.01)]
        vals = _lib.cei_from_moments(ctx, *big, th, mode[0], PAR, mode[1])[0]
        assert _bits(vals[130:130 + m][::-1], base[mode]), mode
        assert _bits(_lib.cei_from_moments(ctx, *big, th, mode[0], PAR, mode[1])[0], vals)
    # refusals: the status, nothing launched
    C17 = _lib.CEI_MAX_CONSTRAINTS + 1
    with pytest.raises(ValueError):
        _lib.cei_from_moments(ctx, mu0, v0, np.zeros((C17, m)), np.ones((C17, m)), np.zeros(C17), "ei", 0.0, 0.45)
    ok16 = _lib.cei_from_moments(ctx, mu0, v0, np.zeros((16, m)), np.ones((16, m)), np.ones(16), "ei", 0.0, 0.45)[0]
    assert np.all(np.isfinite(ok16))
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            _lib.cei_from_moments(ctx, mu0, v0, means, vars_, [0.25, bad], "ei", 0.0, 0.45)
        with pytest.raises(ValueError):
            _lib.cei_from_moments(ctx, mu0, v0, means, vars_, th, "ei", 0.0, bad)
        with pytest.raises(ValueError):
            _lib.cei_from_moments(ctx, mu0, v0, means, vars_, th, "log_ei", bad, 0.45)
    assert _bits(_lib.cei_from_moments(ctx, mu0, v0, means, vars_, th, "ei", PAR, None)[0], base[("ei", None)])
    for kind in ("pi", "lcb", 7, -1):
        with pytest.raises(ValueError):
            _lib.cei_from_moments(ctx, mu0, v0, means, vars_, th, kind, 0.0, 0.45)
    best, out = _lib._Best(), np.empty(m)
    mk, vk = np.ascontiguousarray(means), np.ascontiguousarray(vars_)
    args = [_lib._arr(mu0), _lib._arr(v0), _lib._arr(mk), _lib._arr(vk), _lib._arr(th)]
    call = _lib.lib().robo_cei_eval_moments
    tail = (0, PAR, 0.45, 1, _lib._arr(out)) + best.refs
    for k in range(5):
        a = list(args)
        a[k] = None
        assert call(ctx._h, m, Cn, *a, *tail) == _lib.BAD_ARGUMENT, k
    for bad_c in (-1, C17):
        assert call(ctx._h, m, bad_c, *args, *tail) == _lib.BAD_ARGUMENT
    assert call(None, m, Cn, *args, *tail) == _lib.BAD_ARGUMENT
    assert call(ctx._h, m, Cn, *args, *tail) == _lib.OK and _bits(out, base[("ei", 0.45)])
    worst.report(label + ", chosen cases")
    return worst


# ---- b. the fused form ------------------------------------------------------------------------------------------------------------
def _theta(D, ls2, noise=1e-2, amp=0.0):
    return np.concatenate([[amp], np.log(np.broadcast_to(ls2, (D,))), [np.log(noise)]])


def _fit(ctx, kind, theta, X, y, transform=None):
    g = _lib.DeviceGP(ctx, kind, X.shape[0], X.shape[1])
    g.set_data(X, y)
    if transform is not None:
        g.set_output_transform(*transform)
    g.fit(theta, float(np.mean(y)))
    return g


def _models(ctx, N, D, seed, Cn=3):
    """the objective: Matern-5/2 on N points, raw outputs; the constraints: RBF, fewer points each, an output transform"""
    rs = np.random.RandomState(seed)
    X = rs.rand(N, D)
    y = np.sin(3 * X.sum(axis=1) / np.sqrt(D / 3.0)) + 0.1 * rs.randn(N)
    g0 = _fit(ctx, "matern52", _theta(D, np.array([0.3, 0.5, 0.8, 0.4])[:D]), X, y)
    cons, th = [], []
    for k in range(Cn):
        n = N - 20 - 7 * k
        c = np.cos(2 * X[:n, 0] - X[:n, 1] + k) + 0.5 * (X[:n, -1] - 0.3) ** 2 + 0.1 * rs.randn(n)
        cons.append(_fit(ctx, "rbf", _theta(D, np.array([0.9, 0.6, 0.4, 0.7])[:D] * (1 + 0.2 * k), noise=3e-2, amp=0.3),
                         X[:n], c, transform=(0.7 - k, 2.5 + k)))
        th.append(0.7 - k + (2.5 + k) * 0.2)
    return rs, X, y, g0, cons, np.array(th)


def _check_fused_one(ctx, g0, cons, cand, th, kind, eta, label, worst, rows=None, key=None):
    Cn = len(cons)
    r = g0.cei(cons, cand, th, kind, PAR, eta, diagnostics=True)
    assert r.trace.shape == (cand.m, 2 * (Cn + 1) + 2) and r.values.shape == (cand.m,) and r.flags == 0, label
    # the trace's moments are what robo_gp_predict_cand returns, bit for bit
    for o, g in enumerate([g0] + list(cons)):
        mean, var = g.predict(cand)
        assert _bits(r.trace[:, 2 * o], mean) and _bits(r.trace[:, 2 * o + 1], var), (label, o)
    rows = np.arange(cand.m) if rows is None else np.asarray(rows)
    tr = r.trace[rows]
    mom = (tr[:, 0], tr[:, 1], tr[:, 2:2 * Cn + 2:2].T, tr[:, 3:2 * Cn + 2:2].T)
    # L and the PoF / L alone, the fold on the trace's objective factor, the total
    alone = _oracle(None if key is None else key + ("alone",), *mom, th, kind="log_ei", par=PAR, eta=None)
    worst.take("alone", tr[:, -2], alone, label + " L")
    if eta is not None:
        worst.take("fold", r.values[rows], CO.cei_batch(*mom, th, kind, PAR, eta, obj_dev=tr[:, -1]), label)
    worst.take("alone" if eta is None else "total", r.values[rows],
               _oracle(None if key is None else key + ("total",), *mom, th, kind=kind, par=PAR, eta=eta), label)
    # the moments form on the trace: the same bits
    full = (r.trace[:, 0], r.trace[:, 1], r.trace[:, 2:2 * Cn + 2:2].T, r.trace[:, 3:2 * Cn + 2:2].T)
    vals, mx, am, fl = _lib.cei_from_moments(ctx, *full, th, kind, PAR, eta)
    assert _bits(vals, r.values) and _bits([mx], [r.max]) and am == r.argmax and fl == r.flags, label
    assert r.argmax == CO.np_argmax(r.values) and _bits([r.max], [r.values[r.argmax]]), label
    r2 = g0.cei(cons, cand, th, kind, PAR, eta, diagnostics=True)
    assert _bits(r2.values, r.values) and _bits(r2.trace, r.trace), label
    r3 = g0.cei(cons, cand, th, kind, PAR, eta, want_values=False)
    assert r3.values is None and r3.trace is None and (r3.max, r3.argmax, r3.flags) == (r.max, r.argmax, r.flags), label
    return r


def _check_fused(ctx, label):
    worst = _Worst()
    sz = SMALL
    rs, X, y, g0, cons, th = _models(ctx, sz["N"], sz["D"], 0)
    # the incumbent at the targets' upper quartile: z_0 stays above about -12, where EI's plain form z Phi + phi (which loses
    # z^4 eps to cancellation) is inside what the EI tests grant it; the constraints carry the tails here
    eta = float(np.sort(y)[3 * len(y) // 4])
    Xc_all = rs.rand(max(sz["Ms"]), sz["D"])
    other = _lib.Context(0)
    try:
        for M in sz["Ms"]:
            cand = _lib.Candidates(ctx, Xc_all[:M])
            fresh = _lib.Candidates(ctx, Xc_all[:M])
            try:
                # the plain sweep on a handle no constrained call has touched, and on this one before and after
                plain = {k: (g0.acq(k, PAR, eta, fresh), g0.acq(k, PAR, eta, cand)) for k in ("ei", "log_ei")}
                for kind, e in MODES:
                    e = eta if e is not None else None
                    for Cn in ((3, 1) if M == sz["Ms"][-1] else (3,)):
                        tag = "%s M = %d C = %d %s eta %s" % (label, M, Cn, kind, e)
                        r = _check_fused_one(ctx, g0, cons[:Cn], cand, th[:Cn], kind, e, tag, worst,
                                             key=("fused", label, M, Cn, kind, e is None))
                        assert np.any(r.values != r.values[0]), tag
                    # several passes through a small workspace: the same bits
                    ctx.set_tuning("ws_bytes", 128 * 128 * 8)
                    try:
                        rp = g0.cei(cons, cand, th, kind, PAR, e, diagnostics=True)
                        assert cand.chunk() == 128 and M > 3 * 128
                    finally:
                        ctx.set_tuning("ws_bytes", None)
                    r = g0.cei(cons, cand, th, kind, PAR, e, diagnostics=True)
                    assert _bits(rp.values, r.values) and _bits(rp.trace, r.trace) and rp.argmax == r.argmax, tag
                # C = 0 with an incumbent: robo_acq_eval_cand's bits
                for kind in ("ei", "log_ei"):
                    r0 = g0.cei([], cand, [], kind, PAR, eta, diagnostics=True)
                    assert r0.trace.shape == (M, 4) and _bits(r0.values, plain[kind][0][0]), (M, kind)
                    assert (r0.max, r0.argmax, r0.flags) == plain[kind][0][1:], (M, kind)
                    assert _bits(r0.trace[:, 3], r0.values) and _bits(r0.trace[:, 2], np.zeros(M))
                    after = g0.acq(kind, PAR, eta, cand)
                    for a, b, c in zip(plain[kind][0], plain[kind][1], after):
                        assert _bits([a], [b]) and _bits([a], [c]), (M, kind)
            finally:
                cand.close()
                fresh.close()
        # refusals: nothing is launched, the handles stay usable
        cand = _lib.Candidates(ctx, Xc_all[:64])
        wide = _lib.Candidates(ctx, rs.rand(5, sz["D"] + 1))
        far = _lib.Candidates(other, Xc_all[:5])
        g_far = _fit(other, "rbf", _theta(sz["D"], 0.5), X, y)
        g_wide = _fit(ctx, "rbf", _theta(sz["D"] + 1, 0.5), rs.rand(20, sz["D"] + 1), rs.rand(20))
        raw = _lib.DeviceGP(ctx, "matern52", sz["N"], sz["D"])
        try:
            with pytest.raises(ValueError):
                g0.cei([cons[0], g_far], cand, th[:2], "ei", 0.0, eta)          # a constraint's GP on another context
            with pytest.raises(ValueError):
                g_far.cei(cons[:1], cand, th[:1], "ei", 0.0, eta)               # the objective's GP on another context
            with pytest.raises(ValueError):
                g0.cei(cons, far, th, "ei", 0.0, eta)                            # the candidates on another context
            with pytest.raises(_lib.RoboBadShape):
                g0.cei(cons, wide, th, "ei", 0.0, eta)
            with pytest.raises(_lib.RoboBadShape):
                g0.cei([cons[0], g_wide], cand, th[:2], "ei", 0.0, eta)
            for a, b in ((raw, cons), (g0, [cons[0], raw, cons[1]])):
                with pytest.raises(Exception, match="trained first"):
                    a.cei(b, cand, th[:len(b)], "ei", 0.0, eta)
            with pytest.raises(ValueError):
                g0.cei(cons * 6, cand, np.tile(th, 6), "ei", 0.0, eta)           # 18 constraints
            for bad in (np.nan, np.inf):
                with pytest.raises(ValueError):
                    g0.cei(cons, cand, [th[0], bad, th[2]], "ei", 0.0, eta)
                with pytest.raises(ValueError):
                    g0.cei(cons, cand, th, "ei", 0.0, bad)
                with pytest.raises(ValueError):
                    g0.cei(cons, cand, th, "log_ei", bad, eta)
            for kind in ("pi", "lcb"):
                with pytest.raises(ValueError):
                    g0.cei(cons, cand, th, kind, 0.0, eta)
            best = _lib._Best()
            call = _lib.lib().robo_cei_eval_cand
            hs, tharr = _lib._handles(cons), np.ascontiguousarray(th)
            mid = (0, 0.0, eta, 1)
            assert call(None, hs, 3, _lib._arr(tharr), *mid, cand._h, None, *best.refs, None) == _lib.BAD_ARGUMENT
            assert call(g0._h, None, 3, _lib._arr(tharr), *mid, cand._h, None, *best.refs, None) == _lib.BAD_ARGUMENT
            assert call(g0._h, hs, 3, None, *mid, cand._h, None, *best.refs, None) == _lib.BAD_ARGUMENT
            assert call(g0._h, hs, 3, _lib._arr(tharr), *mid, None, None, *best.refs, None) == _lib.BAD_ARGUMENT
            assert call(g0._h, hs, -1, _lib._arr(tharr), *mid, cand._h, None, *best.refs, None) == _lib.BAD_ARGUMENT
            holes = (_lib.C.c_void_p * 3)(cons[0]._h, None, cons[2]._h)
            assert call(g0._h, holes, 3, _lib._arr(tharr), *mid, cand._h, None, *best.refs, None) == _lib.BAD_ARGUMENT
            ok = g0.cei(cons, cand, th, "ei", 0.0, eta)
            assert ok.flags == 0 and np.all(np.isfinite(ok.values)) and np.all(ok.values >= 0)
        finally:
            for h in (cand, wide, far, g_far, g_wide, raw):
                h.close()
    finally:
        other.close()
        for g in [g0] + cons:
            g.close()
    worst.report(label + ", fused cases")
    return worst


# ---- c. host classes and the front end ----------------------------------------------------------------------------------------------
_BOX = (np.zeros(2), np.ones(2))


def _toy1(x):
    x = np.asarray(x, dtype=np.float64)
    return float(np.sum((x - 0.2) ** 2)), float(1.5 - x[0] - x[1])                 # threshold 0: the corner x0 + x1 >= 1.5


def _toy2(x):
    return _toy1(x) + (float(np.asarray(x)[0] - 0.6),)                              # ... and x0 <= 0.75 (threshold 0.15)


def _gp_models(n=12, seed=0):
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models import GaussianProcess
    rs = np.random.RandomState(seed)
    X = rs.rand(n, 2)
    Y = np.array([_toy2(x) for x in X])
    models = []
    for o, ls in enumerate((0.6, 0.9, 0.7)):
        m = GaussianProcess(Matern52Kernel(np.array([ls, ls]), ndim=2), noise=1e-3, lower=_BOX[0], upper=_BOX[1],
                            normalize_output=bool(o == 1))
        m.train(X, Y[:, o].copy(), do_optimize=False)
        models.append(m)
    return rs, X, Y, models


class _Foreign(object):
    """not a device model for the class: predict() and the training data of a wrapped GP alone (the moments path)"""

    def __init__(self, model, y):
        self._m, self.X, self.y = model, model.X, y
        self.lower, self.upper = model.lower, model.upper

    normalize_input = property(lambda self: self._m.normalize_input)

    def predict(self, X):
        return self._m.predict(X)


_TH2 = np.array([0.6, 0.15])           # the class tests' thresholds: x0 + x1 >= 0.9 and x0 <= 0.75


def _check_class(ctx):
    from robo_amd.acquisition_functions import ConstrainedEI
    from robo_amd.acquisition_functions.constrained_ei import ConstrainedModels, feasible_incumbent, least_violation
    from robo_amd.maximizers import RandomSampling
    from robo_amd.maximizers.random_sampling import DeviceRandomSampling
    worst = _Worst()
    rs, X, Y, models = _gp_models()
    Xc = rs.rand(70, 2)
    for log in (False, True):
        kind = "log_ei" if log else "ei"
        acq = ConstrainedEI(models, _TH2, par=PAR, log=log)
        acq.update(models)
        j = feasible_incumbent(Y[:, 0], Y[:, 1:], _TH2)
        assert j is not None and abs(acq.eta - Y[j, 0]) <= 1e-15 and isinstance(acq.model, ConstrainedModels)
        assert acq.model.objective is models[0] and acq.model.constraints == models[1:] and not hasattr(acq.model, "models")
        x_inc, y_inc = acq.model.get_incumbent()
        assert np.allclose(x_inc, X[j], rtol=0, atol=1e-15) and y_inc == acq.eta
        a = acq.compute(Xc)
        assert a.shape == (70,) and np.all(np.isfinite(a)) and _bits(acq.compute(Xc), a) and _bits(acq(Xc), a)
        i = acq.argmax(Xc)
        assert i == CO.np_argmax(a) == acq.last_argmax and _bits([acq.last_max], [a[i]])
        # the native path against the moments path on the same models, within the bound
        foreign = ConstrainedEI([_Foreign(m, Y[:, o]) for o, m in enumerate(models)], _TH2, par=PAR, log=log)
        assert acq._is_native() and not foreign._is_native() and foreign.eta == Y[j, 0]
        mom = foreign.moments(Xc)
        assert mom[2].shape == (2, 70) and mom[3].shape == (2, 70)
        b = foreign.compute(Xc)
        worst.take("total", b, CO.cei_batch(*mom, _TH2, kind, PAR, foreign.eta), "class, moments path")
        worst.take("total", a, CO.cei_batch(*mom, _TH2, kind, PAR, acq.eta), "class, native path")
        assert foreign.argmax(Xc) == CO.np_argmax(b) == foreign.last_argmax
        # the probability of feasibility: the same rule without the objective, last_max left alone
        keep = (acq.last_max, acq.last_argmax)
        p = acq.probability_of_feasibility(Xc)
        worst.take("alone", p, CO.cei_batch(*mom, _TH2, "ei", PAR, None), "class, PoF")
        assert np.all(p >= 0) and np.all(p <= 1) and (acq.last_max, acq.last_argmax) == keep
        worst.take("alone", foreign.probability_of_feasibility(Xc), CO.cei_batch(*mom, _TH2, "ei", PAR, None), "class, PoF")
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
        dup = copy.deepcopy(acq)
        assert dup.model is not acq.model and _bits(dup.compute(Xc), a) and dup.eta == acq.eta
    # no feasible observation: thresholds nobody meets -> the PoF alone, the incumbent by the smallest largest violation
    hard = np.array([-5.0, -5.0])
    acq = ConstrainedEI(models, hard, par=PAR)
    assert acq.eta is None
    x_inc, y_inc = acq.model.get_incumbent()
    jv = least_violation(Y[:, 1:], hard)
    assert np.allclose(x_inc, X[jv], rtol=0, atol=1e-15) and y_inc == Y[jv, 0]
    assert _bits(acq.compute(Xc), acq.probability_of_feasibility(Xc))
    worst.take("alone", acq.compute(Xc), CO.cei_batch(*ConstrainedEI(models, hard).moments(Xc), hard, "ei", PAR, None),
               "class, none feasible")
    # update() with new thresholds' worth of data: one constraint only
    one = ConstrainedEI(models[:2], _TH2[:1])
    assert one.eta == Y[feasible_incumbent(Y[:, 0], Y[:, 1:2], _TH2[:1]), 0]
    one.update(models[:2])
    assert np.all(np.isfinite(one.compute(Xc)))
    # the maximisers that draw around the incumbent
    acq = ConstrainedEI(models, _TH2)
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
    models[2].devices = [0, 1]
    try:
        for call in (lambda: acq.argmax(Xc), lambda: acq.compute(Xc)):
            with pytest.raises(NotImplementedError, match="devices"):
                call()
    finally:
        models[2].devices = None
    with pytest.raises(ValueError):
        ConstrainedEI(models, _TH2[:1])
    with pytest.raises(ValueError):
        ConstrainedEI(models, [np.nan, 1.0])
    with pytest.raises(ValueError):
        ConstrainedEI([], [])
    with pytest.raises(ValueError):
        ConstrainedEI([models[0], _Foreign(models[1], Y[:-1, 1])], _TH2[:1])
    worst.report("classes")


def _check_class_mcmc(ctx):
    from robo_amd.acquisition_functions import ConstrainedEI
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models.gaussian_process_mcmc import GaussianProcessMCMC
    from robo_amd.priors.default_priors import DefaultPrior
    worst = _Worst()
    rs = np.random.RandomState(2)
    X = rs.rand(10, 2)
    Y = np.array([_toy1(x) for x in X])
    models = []
    for o in range(2):
        kernel = 2 * Matern52Kernel(np.ones(2), ndim=2)
        m = GaussianProcessMCMC(kernel, prior=DefaultPrior(len(kernel) + 1, rng=np.random.RandomState(3 + o)), n_hypers=8,
                                chain_length=4, burnin_steps=2, rng=np.random.RandomState(4 + o), lower=_BOX[0],
                                upper=_BOX[1])
        m.train(X, Y[:, o].copy())
        models.append(m)
    acq = ConstrainedEI(models, [0.6], par=PAR)
    assert not acq._is_native() and acq.eta == Y[Y[:, 1] <= 0.6, 0].min()
    Xc = rs.rand(40, 2)
    a = acq.compute(Xc)
    mom = [np.asarray(v, dtype=np.float64).ravel() for m in models for v in m.predict(Xc)]       # the mixture moments
    worst.take("total", a, CO.cei_batch(mom[0], mom[1], mom[2][None], mom[3][None], [0.6], "ei", PAR, acq.eta),
               "class, gp_mcmc models")
    assert acq.argmax(Xc) == CO.np_argmax(a) and np.all(a >= 0) and a.max() > 0
    worst.report("classes, gp_mcmc")


def _check_front_end(ctx, label):
    """x in [0, 1]^2, f = |x - 0.2|^2, c_1 = 0.9 - x_0 - x_1 <= 0 [, c_2 = x_0 - 0.6 <= 0.15], 3 initial points + 4
    iterations, 60 candidates, seeded.  Every model-based proposal is replayed: the candidates are drawn again from the
    saved random streams, the oracle is evaluated on the models' own moments at them, and the proposal must be the
    oracle's argmax (a pick whose oracle value is within the two bounds of the oracle's maximum counts as that maximum)."""
    from robo_amd.fmin import constrained_optimization
    FE = sys.modules["robo_amd.fmin.constrained_optimization"]      # (the package's attribute of that name is the function)
    from robo_amd.maximizers import RandomSampling
    seen = []

    class Replayed(RandomSampling):
        def maximize(self):
            acq = self.objective_func
            state, own = np.random.get_state(), self.rng.get_state()
            X = self.candidates()
            np.random.set_state(state)
            self.rng.set_state(own)
            x = super(Replayed, self).maximize()                               # draws the same candidates again
            kind = "log_ei" if acq.log else "ei"
            orc = CO.cei_batch(*acq.moments(X), acq.thresholds, kind, acq.par, acq.eta)
            pick = int(np.flatnonzero(np.all(X == x, axis=1))[0])
            best = CO.np_argmax(np.asarray(orc["value"], dtype=np.float64))
            assert pick == best or orc["value"][best] - orc["value"][pick] <= orc["bound"][best] + orc["bound"][pick], \
                (pick, best)
            seen.append((acq.eta, acq.model.y.shape[0]))
            return x

    FE.RandomSampling = Replayed
    try:
        for f, th, acqf, seed in ((_toy1, [0.0], "cei", 1), (_toy2, [0.0, 0.15], "log_cei", 2)):
            del seen[:]
            np.random.seed(seed)
            calls = []

            def g(x):
                calls.append(np.array(x))
                return f(x)
            res = constrained_optimization(g, _BOX[0], _BOX[1], th, num_iterations=7, n_init=3, acquisition_func=acqf,
                                           n_candidates=60, rng=np.random.RandomState(seed))
            X, y, Cv = np.array(res["X"]), np.array(res["y"]), np.array(res["C"])
            assert X.shape == (7, 2) and y.shape == (7,) and Cv.shape == (7, len(th)) and len(calls) == 7 and len(seen) == 4
            assert np.all(X >= _BOX[0]) and np.all(X <= _BOX[1])
            for k in range(7):
                assert (y[k],) + tuple(Cv[k]) == f(X[k])
            feas = np.all(Cv <= np.asarray(th), axis=1)
            assert list(feas) == res["feasible"]
            # incumbents after every evaluation; x_opt / f_opt the best feasible one
            for k in range(7):
                if feas[:k + 1].any():
                    j = int(np.argmin(np.where(feas[:k + 1], y[:k + 1], np.inf)))
                else:
                    j = int(np.argmin(np.max(Cv[:k + 1] - np.asarray(th), axis=1)))
                assert res["incumbents"][k] == X[j].tolist() and res["incumbent_values"][k] == y[j], k
            if feas.any():
                j = int(np.argmin(np.where(feas, y, np.inf)))
                assert res["x_opt"] == X[j].tolist() and res["f_opt"] == y[j]
            else:
                assert res["x_opt"] is None and res["f_opt"] is None
            # PoF-only until the first feasible observation, the weighted form from then on
            for eta, n in seen:
                if feas[:n].any():
                    assert eta == y[:n][feas[:n]].min(), (n, eta)
                else:
                    assert eta is None, (n, eta)
            print("%s: constrained_optimization(%s, C = %d): feasible %s, f_opt %s, incumbents used %s"
                  % (label, acqf, len(th), feas.astype(int).tolist(), res["f_opt"], [e for e, _ in seen]))
            assert len(res["runtime"]) == 7 and len(res["overhead"]) == 7
            assert seen[0][0] is None and seen[-1][0] is not None              # these seeds show the switch
    finally:
        FE.RandomSampling = RandomSampling
    # device_random runs the fused call on device-generated candidates
    np.random.seed(2)
    res = constrained_optimization(_toy1, _BOX[0], _BOX[1], [0.0], num_iterations=5, n_init=3, maximizer="device_random",
                                   n_candidates=128, rng=np.random.RandomState(2))
    assert np.array(res["X"]).shape == (5, 2)
    for kw in (dict(maximizer="scipy"), dict(model_type="rf"), dict(acquisition_func="ei"),
               dict(model_type="gp_mcmc", maximizer="device_random"), dict(model_type="gp_mcmc", hyper_optimizer="device")):
        with pytest.raises(ValueError):
            constrained_optimization(_toy1, _BOX[0], _BOX[1], [0.0], **kw)
    with pytest.raises(ValueError):
        constrained_optimization(_toy1, _BOX[0], _BOX[1], [np.inf])
    with pytest.raises(ValueError):
        constrained_optimization(_toy1, _BOX[0], _BOX[1], [0.0, 0.0], num_iterations=3)      # one value too few returned
    with pytest.raises(AssertionError):
        constrained_optimization(_toy1, _BOX[0], _BOX[1], [0.0], num_iterations=2, n_init=3)
    with pytest.raises(AssertionError):
        constrained_optimization(_toy1, _BOX[1], _BOX[0], [0.0])


def _check_front_end_mcmc(ctx):
    from robo_amd.fmin import constrained_optimization
    np.random.seed(5)
    res = constrained_optimization(_toy1, _BOX[0], _BOX[1], [0.0], num_iterations=4, n_init=3, model_type="gp_mcmc",
                                   n_candidates=60, rng=np.random.RandomState(5), chain_length=4, burnin_steps=2)
    assert np.array(res["X"]).shape == (4, 2) and len(res["feasible"]) == 4 and len(res["incumbent_values"]) == 4


# ---- the runs ----------------------------------------------------------------------------------------------------------------------
def test_moments_emu(emu_ctx):
    _check_moments(emu_ctx, "interpreter")
    _check_moments_special(emu_ctx, "interpreter")


def test_fused_emu(emu_ctx):
    _check_fused(emu_ctx, "interpreter")


def test_classes_emu(emu_ctx):
    _check_class(emu_ctx)
    _check_class_mcmc(emu_ctx)


def test_front_end_emu(emu_ctx):
    _check_front_end(emu_ctx, "interpreter")
    _check_front_end_mcmc(emu_ctx)


@pytest.mark.parametrize("model_type", ["gp", "gp_mcmc"])
def test_front_end_trajectory_emu(emu_ctx, model_type):
    """a seeded run on the interpreter repeats, bit for bit, the trajectory recorded before the front ends' shared loop was
    stated once (tests/golden/fmin_trajectories.json; NOTES.md names the commit): the points ``rng`` is consumed at, and
    every number behind the proposals, are where they were"""
    import json
    from robo_amd.fmin import constrained_optimization
    with open(os.path.join(HERE, "golden", "fmin_trajectories.json")) as f:
        want = json.load(f)["constrained/" + model_type]
    kw = dict(chain_length=4, burnin_steps=2) if model_type == "gp_mcmc" else {}
    np.random.seed(12)
    res = constrained_optimization(_toy1, _BOX[0], _BOX[1], [0.0], num_iterations=5, n_init=3, n_candidates=32,
                                   model_type=model_type, rng=np.random.RandomState(12), **kw)
    assert np.array(res["X"]).shape == (5, 2)
    for key in ("X", "y", "C", "incumbents"):
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
    _check_front_end(gpu_ctx, "MI355X")
    _check_front_end_mcmc(gpu_ctx)


@pytest.mark.gpu
def test_fused_large_gpu(gpu_ctx):
    """N = 256, D = 4, C = 2, m = 32 773: every 97th candidate and the last six against the oracle; the event slots"""
    sz = LARGE
    worst = _Worst()
    rs, X, y, g0, cons, th = _models(gpu_ctx, sz["N"], sz["D"], 4, Cn=2)
    # the incumbent at the targets' upper quartile: z_0 stays above about -12, where EI's plain form z Phi + phi (which loses
    # z^4 eps to cancellation) is inside what the EI tests grant it; the constraints carry the tails here
    eta = float(np.sort(y)[3 * len(y) // 4])
    cand = _lib.Candidates(gpu_ctx, rs.rand(sz["M"], sz["D"]))
    try:
        rows = np.concatenate((np.arange(0, sz["M"], 97), np.arange(sz["M"] - 6, sz["M"])))
        for kind, e in (("ei", eta), ("log_ei", eta), ("ei", None)):
            r = _check_fused_one(gpu_ctx, g0, cons, cand, th, kind, e, "fused large %s %s" % (kind, e), worst, rows)
            assert gpu_ctx.elapsed_ms(32, 33) >= 0.0                       # more than 16 384 candidates: recorded
            assert np.mean(r.trace[:, -2] > -700) > 0.5 and np.any(r.values != r.values[0])
        worst.report("MI355X, fused large")
    finally:
        cand.close()
        for g in [g0] + cons:
            g.close()
