"""Knowledge gradient (robo_amd/csrc/kg.hip, api_kg.hip: robo_kg_eval_cand, robo_kg_eval_marginal_cand,
robo_kg_eval_moments; the KnowledgeGradient class and the "kg" front end) against tests/kg_oracle.py.

CPU: through the interpreter (tests/hipemu).  -m gpu: the same checks at the same small shapes on the MI355X, plus the
fused form at N = 256, D = 4, m = 256 num_cu + 5 (65 541 on the 256-CU part), nb = 50: the cross-covariance takes its
128-row tile when a workspace pass holds at least 2 x num_cu tiles of 128 candidates (infogain.hip launch_cross_cov), and
the test asserts that rule's own inputs.

The oracle is the envelope rule in np.longdouble, itself checked against plain quadrature (test_oracle_against_quadrature).

The value bound.  The device value is compared with the oracle fed THE DEVICE'S OWN DOUBLES (the trace and out_disc_mean,
or the inputs of the moments form); per candidate

    |KG_dev - KG_orc| <= 16 eps sum_k term_k (c_k^2 + 1) + 1e-290 max_j |b_j|

16 = [3.6 (f in fp64, measured against 60-digit arithmetic) + 3 (the breakpoint: two rounded differences and a quotient,
each amplified by the term's conditioning t^2)], doubled.  Largest observed error / (eps sum_k term_k (c_k^2 + 1)):
    interpreter:   2.23 (moments cases), 3.55 (fused cases)
    MI355X:        2.23 (moments cases), 4.41 (fused cases), 2.14 (fused large)
"""
import os
import sys

import numpy as np
import pytest

from robo_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import kg_oracle as KO  # noqa: E402
from _tol import ACQ_RTOL, MU_ATOL, MU_RTOL, VAR_ATOL_REL_AMP  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402

LD = KO.LD
BOUND_FACTOR = 16           # KO.bound
SMALL = dict(N=80, D=3, Ms=(400, 401), nbs=(1, 2, 37, 64), kinds=("matern52", "rbf"))
LARGE = dict(N=256, D=4, nb=50)              # M = 256 num_cu + 5: sized from the device in test_fused_large_gpu


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


# ---- the oracle itself ----------------------------------------------------------------------------------------------------
def test_oracle_against_quadrature():
    """the envelope rule in np.longdouble against the trapezoid rule (2 000 001 nodes on [-12, 12]) of
    min_j(a_j + b_j z) phi(z): 20 random line sets, n in 2 .. 65, equal slopes included"""
    rs = np.random.RandomState(7)
    worst = 0.0
    for case in range(20):
        n = (2, 3, 64, 65)[case] if case < 4 else int(rs.randint(2, 66))
        a, b = rs.randn(n), rs.randn(n)
        if case % 3 == 1:                          # a third of the sets: equal slopes, different intercepts
            b[n // 2:] = b[:n - n // 2]
        kg, _ = KO.envelope(a, b)
        q = KO.quadrature(a, b)
        err = abs(float(kg) - q)
        if abs(float(kg)) >= 1e-9:
            worst = max(worst, err / abs(float(kg)))
        assert err <= 1e-9 * abs(float(kg)) or (abs(float(kg)) < 1e-9 and err <= 1e-9), (case, n, float(kg), q)
    print("oracle against quadrature: worst relative difference %.3e (sets with |KG| >= 1e-9)" % worst)
    # the closed form of two lines, and f at 0: phi(0)
    kg, terms = KO.envelope([0.0, 0.5], [0.0, 2.0])
    assert len(terms) == 1 and abs(float(kg) - 2.0 * float(KO.f_tail(0.25)[0])) < 1e-18
    assert abs(float(KO.f_tail(0.0)[0]) - 0.3989422804014327) < 1e-16


# ---- a. the moments form ---------------------------------------------------------------------------------------------------
class _Worst(object):
    ratio = 0.0


def _check_values(vals, s, v, mu, d, sn2, inc, label, worst, rows=None):
    """every (listed) candidate's value against the oracle on the same doubles, within the bound"""
    rows = range(len(vals)) if rows is None else rows
    sets = [KO.lines(s[c], v[c], mu[c], d, sn2, inc) for c in rows]
    for c, (a, b), (kg, terms) in zip(rows, sets, KO.envelope_batch(sets)):
        if np.isnan(kg):
            assert np.isnan(vals[c]), (label, c)
            continue
        bd, unit = KO.bound(terms, b)
        err = abs(LD(vals[c]) - kg)
        if unit > 0:
            worst.ratio = max(worst.ratio, float(err / unit))
        assert vals[c] >= 0.0 and err <= bd, (label, c, vals[c], float(kg), float(err), float(bd))


def _kg_lines(ctx, a, b, worst, label, self_line=False):
    """the lines a_j + b_j Z of every row (a, b: (n,) or (m, n)) through the moments form: v = 1 and sn2 = 0 make sigma~ = 1,
    so s_j = b_j and the intercepts are the discretisation means (shared by the rows).  self_line: the last line is x
    itself (include_self), whose slope is then v / sigma~ = 1 and whose intercept may differ between the rows."""
    a, b = np.atleast_2d(np.asarray(a, dtype=np.float64)), np.atleast_2d(np.asarray(b, dtype=np.float64))
    m = b.shape[0]
    if self_line:
        assert np.all(b[:, -1] == 1.0) and np.all(a[:, :-1] == a[0, :-1])
        s, d, mu = b[:, :-1], a[0, :-1], a[:, -1]
    else:
        assert np.all(a == a[0])
        s, d, mu = b, a[0], np.zeros(m)
    v = np.ones(m)
    vals, mx, am, fl = _lib.kg_from_moments(ctx, s, v, mu, d, 0.0, self_line)
    _check_values(vals, s, v, mu, d, 0.0, self_line, label, worst)
    assert am == KO.np_argmax(vals) and _bits([mx], [vals[am]]) and fl == 0, label
    return vals


def _check_moments(ctx, label):
    worst = _Worst()
    rs = np.random.RandomState(3)
    # exact zeros: one line; all slopes equal
    vals, mx, am, fl = _lib.kg_from_moments(ctx, rs.randn(5, 1), rs.rand(5) + 0.1, rs.randn(5), rs.randn(1), 0.01, False)
    assert _bits(vals, np.zeros(5)) and am == 0 and mx == 0.0 and fl == 0
    vals, _, _, _ = _lib.kg_from_moments(ctx, np.full((4, 9), 0.37), np.ones(4), rs.randn(4), rs.randn(9), 0.2, False)
    assert _bits(vals, np.zeros(4))
    # two lines: |b_1 - b_0| f(-|a_0 - a_1| / |b_1 - b_0|)
    s, v, mu, d, sn2 = rs.randn(40, 1) * 0.5, rs.rand(40) + 0.05, rs.randn(40), rs.randn(1), 0.03
    vals, _, _, _ = _lib.kg_from_moments(ctx, s, v, mu, d, sn2, True)
    _check_values(vals, s, v, mu, d, sn2, True, "two lines", worst)
    for c in range(40):
        a, b = KO.lines(s[c], v[c], mu[c], d, sn2, True)
        db = abs(b[1] - b[0])
        closed = db * KO.f_tail(abs(a[0] - a[1]) / db)[0]
        assert abs(LD(vals[c]) - closed) <= KO.bound([(db, abs(a[0] - a[1]) / db, closed)], b)[0], ("closed form", c)
    # popped lines: three lines through nearly one point; a dominated line in the middle; n = 2, 3, 64, 65
    z0, y0 = 0.7, -0.3
    b3 = np.array([-1.0, 0.25, 1.0])
    for bump in (0.0, 1e-15, -1e-15, 3e-16):
        a3 = y0 - b3 * z0
        a3[1] += bump
        _kg_lines(ctx, a3, b3, worst, "three lines through nearly one point")
    vals = _kg_lines(ctx, [0.0, 5.0, 0.0], [-1.0, 0.0, 1.0], worst, "dominated middle line")
    assert abs(vals[0] - 2 * 0.3989422804014327) < 1e-15
    for n in (2, 3, 64, 65):
        for rep in range(3):
            a = np.tile(rs.randn(n), (6, 1))
            b = rs.randn(6, n) * (1.0 if rep < 2 else 1e-3)
            if n == 65:
                b[:, -1] = 1.0
                a[:, -1] = rs.randn(6)
            if rep == 1:                                    # lines tangent to a parabola: every one survives
                b = np.tile(np.linspace(-2, 2, n), (6, 1))
                a = 0.25 * b * b
                if n == 65:
                    b, a = b - b[:, -1:] + 1.0, 0.25 * (b - b[:, -1:] + 1.0) ** 2
            _kg_lines(ctx, a, b, worst, "n = %d rep %d" % (n, rep), self_line=n == 65)
    # equal slopes, near-parallel lines, duplicates of a whole line (x coinciding with a z_j)
    _kg_lines(ctx, [0.3, -0.2, 0.9, 0.1], [0.5, 0.5, 0.5, -1.0], worst, "equal slopes, different intercepts")
    _kg_lines(ctx, [0.3, -0.2, 0.1], [0.5, 0.5 * (1 + 2e-16), -1.0], worst, "near-parallel")
    _kg_lines(ctx, [0.3, -0.2, 0.1], [0.5, 0.5 + 1e-9, -1.0], worst, "near-parallel 1e-9")
    s, v, mu, d = np.array([[0.2, 0.8, -0.1]]), np.array([0.8]), np.array([0.4]), np.array([1.0, 0.4, -0.2])
    dup, _, _, _ = _lib.kg_from_moments(ctx, s, v, mu, d, 0.1, True)        # line 1 IS the line of x
    one, _, _, _ = _lib.kg_from_moments(ctx, s, v, mu, d, 0.1, False)
    assert _bits(dup, one)
    _check_values(dup, s, v, mu, d, 0.1, True, "duplicate of a whole line", worst)
    # scale
    _kg_lines(ctx, [0.0, 1e-13, -0.2, 0.1], [1e-12, -1e-12, 1.0, -1.0], worst, "slopes of 1e-12 beside slopes of 1")
    _kg_lines(ctx, [0.0, 1e-13], [1e-12, -1e-12], worst, "slopes of 1e-12 alone")
    big = _kg_lines(ctx, [1e6, 1e6 + 2.0 ** -30], [0.0, 3e-9], worst, "intercepts of 1e6, KG near 1e-9")
    assert 1e-10 < big[0] < 1e-8
    far = _kg_lines(ctx, [0.0, 100.0, -50.0, 37.0], [0.0, 1.0, -1.0, 0.5], worst, "all |c| > 36")
    assert _bits(far, [0.0])
    print("%s: moments cases, largest error / (eps sum term (c^2 + 1)) = %.3g" % (label, worst.ratio))
    assert worst.ratio <= BOUND_FACTOR
    return worst.ratio


def _check_moments_special(ctx):
    rs = np.random.RandomState(5)
    m, nb = 300, 7
    s, v, mu, d = rs.randn(m, nb) * 0.3, rs.rand(m) + 0.1, rs.randn(m), rs.randn(nb)
    base, mx, am, fl = _lib.kg_from_moments(ctx, s, v, mu, d, 0.02, True)
    assert fl == 0 and np.all(np.isfinite(base))
    # NaN in each input in turn: NaN value, the flag, argmax on the first NaN
    for what in ("v", "mean", "s", "disc"):
        s2, v2, mu2, d2 = s.copy(), v.copy(), mu.copy(), d.copy()
        if what == "v":
            v2[[40, 200]] = np.nan
        elif what == "mean":
            mu2[[40, 200]] = np.nan
        elif what == "s":
            s2[40, 3] = s2[200, 0] = np.nan
        else:
            d2[2] = np.nan
        for inc in (True, False):
            vals, mx, am, fl = _lib.kg_from_moments(ctx, s2, v2, mu2, d2, 0.02, inc)
            bad = np.arange(m) if what == "disc" else np.array([40, 200])
            assert np.all(np.isnan(vals[bad])) and np.isnan(vals).sum() == len(bad), (what, inc)
            assert fl == _lib.FLAG_NAN and np.isnan(mx) and am == bad[0], (what, inc, am, fl)
    # ties in the maximum go to the first index
    i = KO.np_argmax(base)
    j = 250 if i < 250 else 100
    s2, v2, mu2 = s.copy(), v.copy(), mu.copy()
    s2[j], v2[j], mu2[j] = s[i], v[i], mu[i]
    vals, mx, am, fl = _lib.kg_from_moments(ctx, s2, v2, mu2, d, 0.02, True)
    assert vals[i] == vals[j] == mx and am == min(i, j)
    # the same candidate row at positions 0, 1, 127, 128, m - 1: the same bits; two calls: the same bits
    s2, v2, mu2 = s.copy(), v.copy(), mu.copy()
    pos = [0, 1, 127, 128, m - 1]
    s2[pos], v2[pos], mu2[pos] = s[77], v[77], mu[77]
    vals, _, _, _ = _lib.kg_from_moments(ctx, s2, v2, mu2, d, 0.02, True)
    assert all(_bits([vals[p]], [base[77]]) for p in pos)
    again = _lib.kg_from_moments(ctx, s2, v2, mu2, d, 0.02, True)
    assert _bits(again[0], vals)
    # argument errors
    for nb_bad in (0, 65):
        with pytest.raises(ValueError):
            _lib.kg_from_moments(ctx, np.zeros((3, nb_bad)), np.ones(3), np.zeros(3), np.zeros(nb_bad), 0.0)
    for sn2 in (-1e-9, np.nan):
        with pytest.raises(ValueError):
            _lib.kg_from_moments(ctx, s, v, mu, d, sn2)
    best = _lib._Best()
    out = np.empty(m)
    args = [_lib._arr(s), _lib._arr(v), _lib._arr(mu), _lib._arr(d)]
    for k in range(4):
        a = list(args)
        a[k] = None
        assert _lib.lib().robo_kg_eval_moments(ctx._h, m, nb, 0.02, 1, *a, _lib._arr(out), *best.refs) == _lib.BAD_ARGUMENT
    assert _lib.lib().robo_kg_eval_moments(None, m, nb, 0.02, 1, *args, _lib._arr(out), *best.refs) == _lib.BAD_ARGUMENT


# ---- b. the fused forms ----------------------------------------------------------------------------------------------------
def _theta(D, ls2, noise=1e-2):
    return np.concatenate([[0.0], np.log(np.broadcast_to(ls2, (D,))), [np.log(noise)]])


def _ls2(D):
    return np.array([0.3, 0.5, 0.8, 0.4])[:D]


def _data(N, D, seed):
    rs = np.random.RandomState(seed)
    X = rs.rand(N, D)
    y = np.sin(3 * X.sum(axis=1) / np.sqrt(D / 3.0)) + 0.1 * rs.randn(N)
    return rs, X, y


def _fit(ctx, kind, theta, X, y):
    g = _lib.DeviceGP(ctx, kind, X.shape[0], X.shape[1])
    g.set_data(X, y)
    g.fit(theta, float(np.mean(y)))
    return g


_ORACLE = {}


def _oracle_posterior(kind, theta, X, y, Xc, Z, key):
    """oracle.gp_oracle's UNCLIPPED full posterior of [Xc; Z], computed once per case and shared"""
    if key not in _ORACLE:
        L = O.gp_compute(kind, theta, X)
        mu, cov = O.gp_predict(kind, theta, L, X, y, float(np.mean(y)), np.concatenate((Xc, Z), axis=0))
        k = Xc.shape[0]
        out = dict(s=cov[:k, k:], v=np.diag(cov)[:k].copy(), mu=mu[:k], disc=mu[k:])
        for a in out.values():
            a.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def _check_trace(r, orc, amp, label, rows=slice(None)):
    nb = r.disc_mean.shape[-1]
    tr = r.trace[rows]
    np.testing.assert_allclose(tr[:, :nb], orc["s"], rtol=0, atol=VAR_ATOL_REL_AMP * amp, err_msg=label)
    np.testing.assert_allclose(tr[:, nb], np.maximum(orc["v"], np.finfo(float).eps), rtol=0, atol=VAR_ATOL_REL_AMP * amp,
                               err_msg=label)
    np.testing.assert_allclose(tr[:, nb + 1], orc["mu"], rtol=MU_RTOL, atol=MU_ATOL, err_msg=label)
    np.testing.assert_allclose(r.disc_mean, orc["disc"], rtol=MU_RTOL, atol=MU_ATOL, err_msg=label)


def _check_fused_one(ctx, g, cand, rep, sn2, inc, label, worst, rows=None):
    """one diagnostics call: values against the oracle on the trace, the moments form on the trace bit for bit, two calls
    and want_values=False"""
    nb = rep.m
    r = g.kg(cand, rep, sn2, inc, diagnostics=True)
    assert r.trace.shape == (cand.m, nb + 2) and r.disc_mean.shape == (nb,) and r.flags == 0, label
    s, v, mu = r.trace[:, :nb], r.trace[:, nb], r.trace[:, nb + 1]
    _check_values(r.values, s, v, mu, r.disc_mean, sn2, inc, label, worst, rows)
    vals, mx, am, fl = _lib.kg_from_moments(ctx, s, v, mu, r.disc_mean, sn2, inc)
    assert _bits(vals, r.values) and _bits([mx], [r.max]) and am == r.argmax and fl == r.flags, label
    assert r.argmax == KO.np_argmax(r.values) and _bits([r.max], [r.values[r.argmax]]), label
    r2 = g.kg(cand, rep, sn2, inc, diagnostics=True)
    assert _bits(r2.values, r.values) and _bits(r2.trace, r.trace) and _bits(r2.disc_mean, r.disc_mean), label
    r3 = g.kg(cand, rep, sn2, inc, want_values=False)
    assert r3.values is None and r3.trace is None and r3.argmax == r.argmax and _bits([r3.max], [r.max]), label
    return r


def _check_fused(ctx, label):
    worst = _Worst()
    sz = SMALL
    sn2 = 1e-2
    for kind in sz["kinds"]:
        rs, X, y = _data(sz["N"], sz["D"], 0)
        theta = _theta(sz["D"], _ls2(sz["D"]))
        g = _fit(ctx, kind, theta, X, y)
        Xc_all, Z_all = rs.rand(max(sz["Ms"]), sz["D"]), rs.rand(max(sz["nbs"]), sz["D"])
        try:
            for M in sz["Ms"]:
                cand = _lib.Candidates(ctx, Xc_all[:M])
                for nb in sz["nbs"]:
                    rep = _lib.Candidates(ctx, Z_all[:nb])
                    tag = "%s %s M = %d nb = %d" % (label, kind, M, nb)
                    try:
                        inc = (nb + M) % 2 == 0 or nb == 1
                        r = _check_fused_one(ctx, g, cand, rep, sn2, inc, tag, worst)
                        orc = _oracle_posterior(kind, theta, X, y, Xc_all, Z_all, (kind, "small"))
                        sub = dict(s=orc["s"][:M, :nb], v=orc["v"][:M], mu=orc["mu"][:M], disc=orc["disc"][:nb])
                        _check_trace(r, sub, 1.0, tag)
                        if nb >= 37:                        # the sign is there: the oracle's own covariance goes negative
                            assert sub["s"].min() < -1e-6 and r.trace[:, :nb].min() < -1e-6, (tag, sub["s"].min())
                    finally:
                        rep.close()
                cand.close()
        finally:
            g.close()
    print("%s: fused cases, largest error / (eps sum term (c^2 + 1)) = %.3g" % (label, worst.ratio))
    assert worst.ratio <= BOUND_FACTOR
    return worst.ratio


def _ep_state(nb, rs):
    logP = np.log(np.full(nb, 1.0 / nb))
    return _lib.EPState(logP, rs.randn(nb), np.linspace(-2, 2, 12), 0.1 * rs.randn(nb, nb),
                        0.1 * rs.randn(nb, nb * (nb + 1) // 2), 0.01 * rs.randn(nb, nb, nb))


def _check_fused_state(ctx):
    """the marginal form, the cached solve of the discretisation across a refit, the clipped path around a KG call, errors"""
    rs, X, y = _data(80, 3, 11)
    S, nb, M = 3, 9, 130
    thetas = []
    for s in range(S):
        th = _theta(3, _ls2(3) * (0.8 + 0.2 * s), noise=1e-2 * (1 + s))
        th[0] = 0.1 * s
        thetas.append(th)
    gps = [_fit(ctx, "matern52", th, X, y) for th in thetas]
    sn2s = np.array([1e-2 * (1 + s) for s in range(S)])
    cand, rep = _lib.Candidates(ctx, rs.rand(M, 3)), _lib.Candidates(ctx, rs.rand(nb, 3))
    try:
        rm = _lib.kg_marginal(gps, cand, rep, sn2s, True, diagnostics=True)
        assert rm.trace.shape == (S, M, nb + 2) and rm.disc_mean.shape == (S, nb)
        total = None
        for s, g in enumerate(gps):
            r = g.kg(cand, rep, sn2s[s], True, diagnostics=True)
            assert _bits(rm.trace[s], r.trace) and _bits(rm.disc_mean[s], r.disc_mean), s
            total = r.values if total is None else total + r.values
        assert len({rm.disc_mean[s].tobytes() for s in range(S)}) == S          # every sample has its own posterior
        assert _bits(rm.values, total / S)
        assert rm.argmax == KO.np_argmax(rm.values) and _bits([rm.max], [rm.values[rm.argmax]])
        rm2 = _lib.kg_marginal(gps, cand, rep, sn2s, True, want_values=False)
        assert rm2.values is None and rm2.argmax == rm.argmax and _bits([rm2.max], [rm.max])
        one = _lib.kg_marginal(gps[:1], cand, rep, sn2s[:1], True, diagnostics=True)
        r0 = gps[0].kg(cand, rep, sn2s[0], True, diagnostics=True)
        assert _bits(one.values, r0.values) and _bits(one.trace[0], r0.trace) and _bits(one.disc_mean[0], r0.disc_mean)
        assert one.argmax == r0.argmax and _bits([one.max], [r0.max])
        # the clipped path (entropy search on the same handles) keeps its bits around a KG call
        ep = _ep_state(nb, rs)
        before = _lib.ig_eval(gps[0], cand, rep, ep, sn2s[0])
        cov_before = _lib.cross_cov(gps[0], cand, rep)
        assert cov_before.min() == np.finfo(float).eps                         # (the clip is active here)
        r0b = gps[0].kg(cand, rep, sn2s[0], True)
        assert _bits(r0b.values, r0.values) and r0.trace[:, :nb].min() < 0
        after = _lib.ig_eval(gps[0], cand, rep, ep, sn2s[0])
        assert _bits(before[0], after[0]) and _bits([before[1]], [after[1]]) and before[2] == after[2]
        assert _bits(cov_before, _lib.cross_cov(gps[0], cand, rep))
        # a refit with a new theta: the cached solve of the discretisation is not used again
        r_old = gps[0].kg(cand, rep, sn2s[0], True)
        gps[0].fit(thetas[1], float(np.mean(y)))
        r_new = gps[0].kg(cand, rep, sn2s[0], True, diagnostics=True)
        fresh = _lib.Candidates(ctx, rep.points())
        try:
            r_fresh = gps[0].kg(cand, fresh, sn2s[0], True, diagnostics=True)
        finally:
            fresh.close()
        assert _bits(r_new.values, r_fresh.values) and _bits(r_new.disc_mean, r_fresh.disc_mean)
        assert _bits(r_new.disc_mean, gps[1].kg(cand, rep, sn2s[0], True).disc_mean) and not _bits(r_new.values, r_old.values)
        # errors
        raw = _lib.DeviceGP(ctx, "matern52", 80, 3)
        wide, rep4 = _lib.Candidates(ctx, rs.rand(65, 3)), _lib.Candidates(ctx, rs.rand(5, 4))
        other = _lib.Context(0)
        far = _lib.Candidates(other, rs.rand(5, 3))
        try:
            with pytest.raises(Exception, match="trained first"):
                raw.kg(cand, rep, 0.0)
            with pytest.raises(ValueError):
                gps[0].kg(cand, wide, 0.0)                                     # nb = 65
            for bad in (-1.0, np.nan):
                with pytest.raises(ValueError):
                    gps[0].kg(cand, rep, bad)
            for r_bad in (rep4, far):
                with pytest.raises(_lib.RoboBadShape):
                    gps[0].kg(cand, r_bad, 0.0)
            gps[2].set_precision(True)
            gps[2].fit(thetas[2], float(np.mean(y)))
            with pytest.raises(ValueError):
                gps[2].kg(cand, rep, 0.0)                                      # fp32 covariance entries
            best = _lib._Best()
            assert _lib.lib().robo_kg_eval_cand(gps[0]._h, cand._h, None, 0.0, 1, None, *best.refs, None, None) \
                == _lib.BAD_ARGUMENT
            ok = gps[1].kg(cand, rep, sn2s[1], True)                           # a refused call leaves the handles usable
            assert ok.flags == 0 and np.all(np.isfinite(ok.values))
        finally:
            far.close()
            other.close()
            rep4.close()
            wide.close()
            raw.close()
    finally:
        cand.close()
        rep.close()
        for g in gps:
            g.close()


# ---- c. host classes and the front end ---------------------------------------------------------------------------------------
def _branin(x):
    a, b, c, r, s, t = 1.0, 5.1 / (4 * np.pi ** 2), 5.0 / np.pi, 6.0, 10.0, 1.0 / (8 * np.pi)
    return float(a * (x[1] - b * x[0] ** 2 + c * x[0] - r) ** 2 + s * (1 - t) * np.cos(x[0]) + s)


_BOX = (np.array([-5.0, 0.0]), np.array([10.0, 15.0]))


def _gp_model(seed=0, n=12, ls=0.5, noise=1e-3):
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models import GaussianProcess
    rs = np.random.RandomState(seed)
    X = _BOX[0] + (_BOX[1] - _BOX[0]) * rs.rand(n, 2)
    y = np.array([_branin(x) for x in X]) / 50.0
    model = GaussianProcess(Matern52Kernel(np.array([ls, ls]), ndim=2), noise=noise, lower=_BOX[0], upper=_BOX[1])
    model.train(X, y, do_optimize=False)
    return rs, model


class _ForeignModel(object):
    """not a device model for the class: predict() and predict(full_cov=True) of a wrapped GP alone (the moments path)"""

    def __init__(self, model):
        self._m = model
        self.lower, self.upper, self.X = model.lower, model.upper, None

    def predict(self, X, full_cov=False):
        return self._m.predict(X, full_cov=full_cov)

    def get_noise(self):
        return self._m.get_noise()


def _check_class(ctx):
    from robo_amd.acquisition_functions import KnowledgeGradient
    from robo_amd.maximizers import RandomSampling, SciPyOptimizer
    from robo_amd.maximizers.random_sampling import DeviceRandomSampling
    lo, hi = _BOX
    # a weakly informative model: every posterior covariance involved stays above the floor predict(full_cov=True) applies,
    # so the clipped moments of the generic path and the signed ones of the fused call are the same numbers
    rs, model = _gp_model(ls=4.0, noise=10.0)
    acq = KnowledgeGradient(model, n_disc=9, n_grid=120, rng=np.random.RandomState(3))
    acq.update(model)
    Xc = lo + (hi - lo) * rs.rand(70, 2)
    a = acq.compute(Xc)
    Z = acq.discretisation_points()
    assert a.shape == (70,) and np.all(a >= 0) and np.all(np.isfinite(a)) and Z.shape == (9, 2)
    assert _bits(acq.compute(Xc), a)
    cand = _lib.Candidates(model.gp.ctx, model._normalised(Xc))
    try:
        assert _bits(acq.compute(cand), a)                                    # a device batch is the same call
        assert acq.argmax(cand) == KO.np_argmax(a)
        model.normalize_input = False
        try:
            with pytest.raises(TypeError):
                acq.compute(cand)
        finally:
            model.normalize_input = True
    finally:
        cand.close()
    mu, cov = model.predict(np.concatenate((Xc, Z)), full_cov=True)
    assert cov.min() > 1e-6                                                   # the floor is nowhere near
    vals, mx, am, _ = _lib.kg_from_moments(ctx, cov[:70, 70:], np.diag(cov)[:70], mu[:70], mu[70:], model.get_noise(), True)
    np.testing.assert_allclose(a, vals, rtol=ACQ_RTOL, atol=0)
    foreign = KnowledgeGradient(_ForeignModel(model), discretisation=Z)       # ... which is what a foreign model gets
    assert _bits(foreign.compute(Xc), vals) and foreign.argmax(Xc) == am == foreign.last_argmax
    i = acq.argmax(Xc)
    assert i == KO.np_argmax(a) == acq.last_argmax and _bits([acq.last_max], [a[i]])
    # the default discretisation: lowest posterior means of the grid, reproducible from the rng; new after update()
    again = KnowledgeGradient(model, n_disc=9, n_grid=120, rng=np.random.RandomState(3))
    again.update(model)
    assert _bits(again.discretisation_points(), Z) and _bits(again.compute(Xc), a)
    from robo_amd.acquisition_functions.max_value_entropy_search import mes_grid
    G = mes_grid(model, np.random.RandomState(3), 120)                        # 120 uniform points + the training inputs
    assert G.shape == (120 + 12, 2) and _bits(Z, G[np.argsort(model.predict(G)[0], kind="stable")[:9]])
    acq.update(model)
    assert not _bits(acq.discretisation_points(), Z)
    # discretisation= is honoured
    Zg = lo + (hi - lo) * rs.rand(5, 2)
    given = KnowledgeGradient(model, discretisation=Zg, include_self=False)
    given.update(model)
    g = given.compute(Xc)
    assert _bits(given.discretisation_points(), Zg)
    rep = _lib.Candidates(model.gp.ctx, model._normalised(Zg))
    cand = _lib.Candidates(model.gp.ctx, model._normalised(Xc))
    try:
        assert _bits(g, model.gp.kg(cand, rep, model.get_noise(), False).values)
    finally:
        rep.close()
        cand.close()
    for bad in (np.zeros((65, 2)), np.zeros(3)):
        with pytest.raises(ValueError):
            KnowledgeGradient(model, discretisation=bad)
    with pytest.raises(ValueError):
        KnowledgeGradient(model, n_disc=65)
    # every maximiser, the single-point ones included
    for mk in (lambda: RandomSampling(acq, lo, hi, n_samples=60), lambda: DeviceRandomSampling(acq, lo, hi, n_samples=128,
               rng=np.random.RandomState(9)), lambda: SciPyOptimizer(acq, lo, hi, n_restarts=2, rng=np.random.RandomState(2))):
        x = mk().maximize()
        assert x.shape == (2,) and np.all(x >= lo) and np.all(x <= hi)
    # both refusals
    with pytest.raises(NotImplementedError):
        acq.compute(Xc, derivative=True)
    model.devices = [0, 1]
    try:
        for call in (lambda: acq.argmax(Xc), lambda: acq.compute(Xc), lambda: (acq.update(model), acq.compute(Xc))):
            with pytest.raises(NotImplementedError, match="devices"):
                call()
    finally:
        model.devices = None
    with pytest.raises(NotImplementedError):
        acq.argmax_sharded(None, Xc[:10], 0)


def _check_class_marginal(ctx):
    from robo_amd.acquisition_functions import KnowledgeGradient
    from robo_amd.acquisition_functions.marginalization import MarginalizationGPMCMC
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models.gaussian_process_mcmc import GaussianProcessMCMC
    from robo_amd.priors.default_priors import DefaultPrior
    rs = np.random.RandomState(2)
    X = _BOX[0] + (_BOX[1] - _BOX[0]) * rs.rand(14, 2)
    y = np.array([_branin(x) for x in X]) / 50.0
    kernel = 2 * Matern52Kernel(np.ones(2), ndim=2)
    model = GaussianProcessMCMC(kernel, prior=DefaultPrior(len(kernel) + 1, rng=np.random.RandomState(3)), n_hypers=8,
                                chain_length=6, burnin_steps=4, rng=np.random.RandomState(4), lower=_BOX[0], upper=_BOX[1])
    model.train(X, y)
    acq = MarginalizationGPMCMC(KnowledgeGradient(model, n_disc=7, n_grid=100, rng=np.random.RandomState(5)))
    acq.update(model)
    assert acq._kg_native()
    Xc = _BOX[0] + (_BOX[1] - _BOX[0]) * rs.rand(90, 2)
    a = acq.compute(Xc)
    S = len(acq.estimators)
    assert S > 1 and a.shape == (90,) and _bits(acq.compute(Xc), a)
    # the per-sample mean over the shared discretisation, accumulated in sample order
    total = np.zeros(90)
    for e in acq.estimators:
        total = total + e.compute(Xc)
    assert _bits(a, total / S)
    i = acq.argmax(Xc)
    assert i == KO.np_argmax(a) == acq.last_argmax and _bits([acq.last_max], [a[i]])
    Z = acq.estimators[0].discretisation_points()
    acq.update(model)
    assert all(e._disc is None for e in acq.estimators) and acq._kg_rep is None
    assert not _bits(acq.compute(Xc), a) and not _bits(acq.estimators[0].discretisation_points(), Z)
    with pytest.raises(NotImplementedError):
        acq.compute(Xc, derivative=True)
    acq.sample_shard = True
    try:
        with pytest.raises(NotImplementedError):
            acq.compute(Xc)
    finally:
        acq.sample_shard = False
    model.devices = [0, 1]
    try:
        with pytest.raises(NotImplementedError, match="devices"):
            acq.argmax(Xc)
    finally:
        model.devices = None


def _bo(model_type, seed=3, **kw):
    from robo_amd.fmin import bayesian_optimization
    np.random.seed(seed)
    calls = []

    def f(x):
        calls.append(np.array(x))
        return _branin(x)
    res = bayesian_optimization(f, _BOX[0], _BOX[1], num_iterations=6, maximizer="random", acquisition_func="kg",
                                model_type=model_type, n_init=3, rng=np.random.RandomState(seed), n_candidates=150, **kw)
    return res, np.array(calls)


def _check_front_end(ctx):
    for model_type, kw in (("gp", {}), ("gp_mcmc", dict(chain_length=6, burnin_steps=4))):
        a, ca = _bo(model_type, **kw)
        assert ca.shape == (6, 2)                                              # the objective once per iteration
        assert np.all(np.isfinite(ca)) and np.all(np.isfinite(a["y"])) and np.isfinite(a["f_opt"])
        assert np.all(np.isfinite(a["x_opt"])) and np.all(ca >= _BOX[0]) and np.all(ca <= _BOX[1])


# ---- the runs ------------------------------------------------------------------------------------------------------------------
def test_moments_emu(emu_ctx):
    _check_moments(emu_ctx, "interpreter")
    _check_moments_special(emu_ctx)


def test_fused_emu(emu_ctx):
    _check_fused(emu_ctx, "interpreter")


def test_fused_state_emu(emu_ctx):
    _check_fused_state(emu_ctx)


def test_class_emu(emu_ctx):
    _check_class(emu_ctx)


def test_class_marginal_emu(emu_ctx):
    _check_class_marginal(emu_ctx)


def test_front_end_emu(emu_ctx):
    _check_front_end(emu_ctx)


@pytest.mark.gpu
def test_moments_gpu(gpu_ctx):
    _check_moments(gpu_ctx, "MI355X")
    _check_moments_special(gpu_ctx)


@pytest.mark.gpu
def test_fused_gpu(gpu_ctx):
    _check_fused(gpu_ctx, "MI355X")


@pytest.mark.gpu
def test_fused_state_gpu(gpu_ctx):
    _check_fused_state(gpu_ctx)


@pytest.mark.gpu
def test_classes_and_front_end_gpu(gpu_ctx):
    _check_class(gpu_ctx)
    _check_class_marginal(gpu_ctx)
    _check_front_end(gpu_ctx)


@pytest.mark.gpu
def test_fused_large_gpu(gpu_ctx):
    """a chunk of at least 2 x num_cu tiles of 128 candidates (2 num_cu + 1 of them, the last one ragged): the
    cross-covariance's 128-row tile, signed.  num_cu is the device's multiprocessor count, the number the library reads
    (torch's device properties, asked in a child process: vcons_checks.device_cu_count)."""
    from vcons_checks import device_cu_count
    num_cu = device_cu_count()
    sz = dict(LARGE, M=256 * num_cu + 5)
    worst = _Worst()
    rs, X, y = _data(sz["N"], sz["D"], 4)
    theta = _theta(sz["D"], _ls2(sz["D"]))
    g = _fit(gpu_ctx, "matern52", theta, X, y)
    Xc, Z = rs.rand(sz["M"], sz["D"]), rs.rand(sz["nb"], sz["D"])
    cand, rep = _lib.Candidates(gpu_ctx, Xc), _lib.Candidates(gpu_ctx, Z)
    try:
        rows = np.concatenate((np.arange(0, sz["M"], 97), np.arange(sz["M"] - 6, sz["M"])))
        r = _check_fused_one(gpu_ctx, g, cand, rep, 1e-2, True, "fused large", worst, rows)
        assert cand.chunk() // 128 >= 2 * num_cu, (cand.chunk(), num_cu)        # launch_cross_cov's rule for the 128-row tile
        orc = _oracle_posterior("matern52", theta, X, y, Xc[rows], Z, "large")
        _check_trace(r, orc, 1.0, "fused large", rows)
        assert orc["s"].min() < -1e-6 and r.trace[:, :sz["nb"]].min() < -1e-6
        print("MI355X: fused large, largest error / (eps sum term (c^2 + 1)) = %.3g" % worst.ratio)
        assert worst.ratio <= BOUND_FACTOR
    finally:
        cand.close()
        rep.close()
        g.close()
