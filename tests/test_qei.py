"""Joint Monte-Carlo batch EI with greedy picks (robo_amd/csrc/qei.hip, robo_qei_batch_cand / robo_qei_batch_marginal_cand,
DeviceGP.select_batch_joint, fantasy="joint") against tests/qei_oracle.py.

Whole selections are not compared.  Every pick is checked on its own, given the device's OWN earlier picks:
  1. moments: out_coef, out_d and the traced (mean, residual var) against the oracle's joint posterior from raw inputs;
  2. values: out_acq against an np.longdouble recomputation from the device's own out_coef, out_d, trace, out_best and z,
     and out_best against min(b, f^k(p_j)) formed from the device's doubles;
  3. decisions: the pick is the first index attaining the maximum of the device's own out_acq, and equals the oracle's
     greedy choice where the oracle shows no near tie.
Every case runs through the interpreter (tests/hipemu) and, with -m gpu, on the MI355X.

Tolerances.  The base errors are those of the same code path in tests/test_batch_select.py (BATCH_MU_ATOL,
BATCH_VAR_ATOL_REL_AMP in units of k(x, x); the _GPU pair for N >= 1024); qei_oracle.bounds propagates them per candidate
through the history term and l^2 = c^2 / d, growing with sqrt(k(x, x) / d_t).  The seeds are chosen so that the ORACLE's
d_t >= 1e-3 k(x, x) at every pick (asserted), which keeps that bound meaningful.
Measured worst cases as a fraction of the bound, over all cases of this file (_check_each_pick prints them per case):
    MI355X:       mean 0.070, residual var 0.12 (the marginalised class), c_t(x) 0.058, d_t 0.058;
                  values 1.6e-8 relative (bound 1e-7)
    interpreter:  mean 0.047, var 0.12, c_t(x) 0.062, d_t 0.044; values 9.3e-9 relative
No base constant of that file had to be widened.  The q = 64 edge, where the propagated bound says nothing, has a
measured absolute one (Q64_REL_AMP).
Values against the longdouble recomputation: bound ACQ_RTOL = 1e-7 relative plus K eps of the sum, plus DBL_MIN absolute
(subnormal terms carry no relative precision; acq_kernel's rule counts them as noise).
"""
import os
import sys

import numpy as np
import pytest

from robo_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import qei_oracle as QO  # noqa: E402
import test_batch_select as TB  # noqa: E402  (the shared helpers and the base tolerances of the conditioning path)
from _tol import ACQ_RTOL  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402

EPS = QO.EPS
SMALL = dict(N=80, D=3, M=400, q=5, K=128)
SEEDS = (0, 1, 2)
GAP = 1e-6                       # the oracle's best-to-second relative gap below which a pick is not compared
DBL_MIN = 2.2250738585072014e-308    # a term below it has no relative precision left (subnormal) and counts as noise in acq_kernel
# the q = 64 edge, 63 steps deep, against the oracle in units of k(x, x): measured 3.4e-15 (c_t), 3.3e-15 (d_t), 3.3e-15
# (residual var) through the interpreter and 1.9e-15, 1.4e-15, 2.6e-15 on the MI355X; the largest times about 10
Q64_REL_AMP = 4e-14
D_MIN = 1e-3                     # the condition on the oracle's d_t / k(x, x)


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def ctx(request):
    if request.param == "emu":
        sys.path.insert(0, os.path.join(HERE, "hipemu"))
        import build_emu
        _lib.use_library(build_emu.build())
        c = _lib.Context(0)
        assert "hipemu" in c.name
        yield c
        c.close()
        _lib.use_library(None)
    else:
        _lib.use_library(None)
        if _lib.device_count() < 1:
            pytest.skip("no HIP device")
        yield _lib.default_context()


def _z(K, q, seed=100):
    return np.random.RandomState(seed).standard_normal((K, q))


def _bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


# ---- the oracle on its own (no device) -------------------------------------------------------------------------------------
def _oracle_case(M=40, seed=3, transform=(0.3, 1.7)):
    rs, X, y = TB._data(60, 3, seed)
    yl = (y - transform[0]) / transform[1]
    og = TB.BO.FrozenGP("matern52", TB._theta(3, [0.3, 0.5, 0.8]), X, yl, float(np.mean(yl)), *transform)
    return og, rs.rand(M, 3), float(y.min())


def test_oracle_q1_is_closed_form_ei():
    og, Xc, eta = _oracle_case()
    post = QO.JointPosterior(og, Xc)
    a, _ = QO.Greedy([post], eta, 0.01, _z(7, 1)).values([])
    m, v = og.refit(Xc, [])
    np.testing.assert_allclose(a.astype(np.float64), O.ei(m, v, eta, 0.01), rtol=1e-9, atol=0)


def test_oracle_rao_blackwell_agrees_with_plain_monte_carlo_and_telescopes():
    og, Xc, eta = _oracle_case()
    post = QO.JointPosterior(og, Xc, dtype=np.float64)
    K, q = 2 ** 16, 3
    gr = QO.Greedy([post], eta, 0.0, _z(K, q, 7))
    picks, gains, _ = gr.run(q)
    assert len(set(picks)) == q
    # the telescoped total, scenario by scenario: gain_0 (closed form) + the winners' terms of picks 1 and 2
    total = np.full(K, float(gains[0]))
    for j in range(1, q):
        Lpp, l, d, var, b = gr.values(picks[:j])[1][0]
        _, terms = QO.fold(post.mean_t, post.var_t(var), l, gr.z, b, og.y_std)
        total += terms[:, picks[j]]
    rb, rb_se = total.mean(), total.std(ddof=1) / np.sqrt(K)
    np.testing.assert_allclose(rb, float(sum(gains)), rtol=1e-12)                     # the increments telescope to it
    plain, plain_se = QO.plain_qei(post, picks, eta, 2 ** 18, np.random.RandomState(11))
    print("q-EI of %r: Rao-Blackwell %.6e +- %.1e, plain %.6e +- %.1e" % (picks, rb, rb_se, plain, plain_se))
    assert abs(rb - plain) <= 5 * np.hypot(rb_se, plain_se)


# ---- every pick on its own ---------------------------------------------------------------------------------------------------
def _device_values(r, j, z, y_stds):
    """every candidate's value at pick j in np.longdouble from the device's own coef, d, trace, best and z"""
    LD = QO.LD
    S = r.trace.shape[1]
    acc = None
    for s in range(S):
        l = np.stack([r.coef[u, s].astype(LD) / np.sqrt(LD(r.d[u, s])) for u in range(j)]) if j else np.zeros((0, r.trace.shape[2]), LD)
        g, _ = QO.fold(r.trace[j, s, :, 0].astype(LD), r.trace[j, s, :, 1].astype(LD), l, z, r.best[j, s].astype(LD), y_stds[s])
        acc = g if acc is None else acc + g
    return acc / LD(S)


def _check_values_and_decisions(r, z, y_stds, label=""):
    """checks 2 and 3a: from the device's own outputs alone"""
    K, worst = z.shape[0], 0.0
    S = r.trace.shape[1]
    for j in range(r.n_made):
        want = _device_values(r, j, z, y_stds).astype(np.float64)
        got = r.acq[j]
        ok = np.isfinite(want)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        err = np.abs(got[ok] - want[ok])
        tol = ACQ_RTOL * np.abs(want[ok]) + K * EPS * np.abs(want[ok]) + DBL_MIN
        worst = max(worst, float((err / np.maximum(np.abs(want[ok]), 1e-300)).max()) if ok.any() else 0.0)
        assert np.all(err <= tol), (label, j, float((err - tol).max()))
        i = int(r.indices[j])
        assert i == O.np_argmax(got), (label, j, i)               # first index, NaN maximal
        assert _bits(r.gains[j], got[i])
        if j + 1 < r.n_made:                                        # b^k after pick j, from the device's doubles
            for s in range(S):
                lp = np.array([r.coef[u, s, i] / np.sqrt(r.d[u, s]) for u in range(j)])
                sd = np.sqrt(r.d[j, s])
                f = r.trace[j, s, i, 0] + y_stds[s] * (z[:, :j] @ lp + sd * z[:, j])
                mag = abs(r.trace[j, s, i, 0]) + y_stds[s] * (np.abs(z[:, :j]) @ np.abs(lp) + sd * np.abs(z[:, j]))
                np.testing.assert_array_less(np.abs(r.best[j + 1, s] - np.minimum(r.best[j, s], f)), 4 * (j + 2) * EPS * mag + 1e-300)
    assert np.all(r.indices[r.n_made:] == -1) and np.all(np.isnan(r.gains[r.n_made:]))
    np.testing.assert_array_equal(r.qei[:r.n_made], np.cumsum(r.gains[:r.n_made]))
    return worst


def _check_each_pick(r, ogs, Xc, z, par, etas, mu_atol, var_rel, label="", dtype=QO.LD, rows=None):
    """every pick of a QEIResult with diagnostics on its own, given the device's own earlier picks.  rows: the candidates the
    oracle is restated on (all of them when None; the picks must be among them) -> (near ties left out, picks compared)"""
    S = len(ogs)
    etas = np.array(np.broadcast_to(etas, (S,)), dtype=np.float64)
    rows = np.arange(Xc.shape[0]) if rows is None else np.asarray(rows)
    at = {int(g): k for k, g in enumerate(rows)}
    posts = [QO.JointPosterior(og, Xc[rows], dtype) for og in ogs]
    gr = QO.Greedy(posts, etas, par, z)
    y_stds = [og.y_std for og in ogs]
    worst = dict(mu=0.0, var=0.0, coef=0.0, d=0.0)
    left_out = 0
    assert r.n_made >= 1
    for j in range(r.n_made):
        picks = [at[int(i)] for i in r.indices[:j]]
        a, state = gr.values(picks)
        for s, (post, (Lpp, l, d, var, b)) in enumerate(zip(posts, state)):
            amp = post.amp.astype(np.float64)
            assert np.all(d.astype(np.float64) >= D_MIN * amp[picks]), (label, j, s, d / amp[picks])
            e_c, e_d, e_v = QO.bounds(post, picks, d, mu_atol, var_rel)
            ys2 = post.gp.y_std ** 2
            dm = np.abs(r.trace[j, s, rows, 0] - post.mean_t.astype(np.float64))
            dv = np.abs(r.trace[j, s, rows, 1] - post.var_t(var).astype(np.float64))
            worst["mu"] = max(worst["mu"], dm.max() / (mu_atol * max(1.0, post.gp.y_std)))
            worst["var"] = max(worst["var"], (dv / (e_v[j] * ys2)).max())
            assert np.all(dm <= mu_atol * max(1.0, post.gp.y_std)), (label, j, s, dm.max())
            assert np.all(dv <= e_v[j] * ys2), (label, j, s, (dv / (e_v[j] * ys2)).max())
            assert _bits(r.trace[j, s, :, 0], r.trace[0, s, :, 0])                       # the mean state is never touched
            assert _bits(r.best[0, s], np.full(z.shape[0], etas[s] - par))
            if j >= 1:
                t = j - 1
                dc = np.abs(r.coef[t, s, rows] - (l[t] * np.sqrt(d[t])).astype(np.float64))
                dd = abs(r.d[t, s] - float(d[t]))
                worst["coef"] = max(worst["coef"], (dc / e_c[t]).max())
                worst["d"] = max(worst["d"], dd / e_d[t])
                assert np.all(dc <= e_c[t]), (label, j, s, (dc / e_c[t]).max())
                assert dd <= e_d[t], (label, j, s, dd, e_d[t])
        i = at[int(r.indices[j])]
        top = np.sort(a)[-2:] if len(a) > 1 else np.array([0.0, 1.0])
        if top[1] - top[0] >= GAP * abs(top[1]):
            assert i == O.np_argmax(a.astype(np.float64)), (label, j, i, O.np_argmax(a.astype(np.float64)))
        else:
            left_out += 1
    if r.n_made:
        assert np.all(np.isnan(r.d[r.n_made - 1]))                  # nothing is conditioned on the last pick made
    v = _check_values_and_decisions(r, z, y_stds, label) if rows.shape[0] == Xc.shape[0] else float("nan")
    print("%s: %d picks; worst error as a fraction of its bound: mean %.2e, var %.2e, coef %.2e, d %.2e; values %.2e relative"
          % (label, r.n_made, worst["mu"], worst["var"], worst["coef"], worst["d"], v))
    return left_out, r.n_made


def _run(g, par, eta, cand, q, z):
    return g.select_batch_joint(par, eta, cand, q, z, diagnostics=True)


def test_every_pick_small(ctx):
    """the issue's shape on three seeds, Matern-5/2, noise 1e-2; at most 1 in 5 (seed, pick) pairs left out for near ties"""
    left = total = 0
    for seed in SEEDS:
        rs, og, g, eta, Xc = TB._setup(ctx, SMALL, seed=seed)
        cand = _lib.Candidates(ctx, Xc)
        try:
            z = _z(SMALL["K"], SMALL["q"], 100 + seed)
            r = _run(g, 0.0, eta, cand, SMALL["q"], z)
            assert r.n_made == SMALL["q"]
            a, b = _check_each_pick(r, [og], Xc, z, 0.0, eta, TB.BATCH_MU_ATOL, TB.BATCH_VAR_ATOL_REL_AMP, "seed %d" % seed)
            left, total = left + a, total + b
            r2 = _run(g, 0.0, eta, cand, SMALL["q"], z)                      # two calls agree; the state is reused
            for name in ("indices", "gains", "flags", "acq", "trace", "coef", "d", "best"):
                assert _bits(getattr(r, name), getattr(r2, name)), name
        finally:
            cand.close()
            g.close()
    assert 5 * left <= total, (left, total)


@pytest.mark.parametrize("kernel,transform,par,noise", [("rbf", (0.0, 1.0), 0.0, 1e-2), ("fabolas", (0.0, 1.0), 0.0, 1e-2),
                                                        ("matern52", (3.0, 2.5), 0.02, 1e-2), ("matern52", (0.0, 1.0), 0.0, 1e-6)],
                         ids=["rbf", "fabolas", "transform+par", "noise1e-6"])
def test_every_pick_kinds_transform_noise(ctx, kernel, transform, par, noise):
    rs, og, g, eta, Xc = TB._setup(ctx, SMALL, kernel, seed=1, noise=noise, transform=transform)
    cand = _lib.Candidates(ctx, Xc)
    mu_atol, var_rel = (TB.BATCH_MU_ATOL, TB.BATCH_VAR_ATOL_REL_AMP) if noise >= 1e-3 else \
        (TB.BATCH_MU_ATOL_NOISE_1E8, TB.BATCH_VAR_ATOL_REL_AMP_NOISE_1E8)     # (the ill-conditioned pair of that file)
    try:
        z = _z(64, 4, 5)
        r = _run(g, par, eta, cand, 4, z)
        assert r.n_made == 4
        _check_each_pick(r, [og], Xc, z, par, eta, mu_atol, var_rel, "%s %r" % (kernel, transform))
    finally:
        cand.close()
        g.close()


def test_marginal(ctx):
    gps, ogs, etas, Xc = TB._marginal_setup(ctx, SMALL, S=3)
    cand = _lib.Candidates(ctx, Xc)
    try:
        z = _z(64, 3, 9)
        r = _lib.qei_batch(gps, 0.0, etas, cand, 3, z, diagnostics=True)
        assert r.n_made == 3 and r.trace.shape[1] == 3
        _check_each_pick(r, ogs, Xc, z, 0.0, etas, TB.BATCH_MU_ATOL, TB.BATCH_VAR_ATOL_REL_AMP, "marginal")
    finally:
        cand.close()
        for g in gps:
            g.close()


# ---- identities, bit for bit ---------------------------------------------------------------------------------------------------
def test_identities(ctx):
    rs, og, g, eta, Xc = TB._setup(ctx, SMALL)
    _, _, g2, _, _ = TB._setup(ctx, SMALL)                                    # the same data and theta
    cand = _lib.Candidates(ctx, Xc)
    z = _z(32, 3, 4)
    try:
        vals, mx, am, fl = g.acq("ei", 0.01, eta, cand, want_values=True)
        _, mx2, am2, fl2 = g.acq("ei", 0.01, eta, cand, want_values=False)
        r1 = _run(g, 0.01, eta, cand, 1, z[:, :1])
        r3 = _run(g, 0.01, eta, cand, 3, z)
        for r in (r1, r3):                                                    # q = 1 and pick 0 of any q: the sweep
            assert r.indices[0] == am == am2 and r.flags[0] == fl == fl2
            assert _bits(r.gains[0], mx) and _bits(r.gains[0], mx2) and _bits(r.acq[0], vals)
        lean = g.select_batch_joint(0.01, eta, cand, 3, z)                     # without diagnostics: the same picks
        assert _bits(lean.indices, r3.indices) and _bits(lean.gains, r3.gains) and lean.acq is None
        # the marginal form with S = 1, and with two identical GPs
        for gps in ([g], [g, g2]):
            rm = _lib.qei_batch(gps, 0.01, eta, cand, 3, z, diagnostics=True)
            assert _bits(rm.indices, r3.indices) and _bits(rm.gains, r3.gains) and _bits(rm.acq, r3.acq)
            assert _bits(rm.trace[:, 0], r3.trace[:, 0]) and _bits(rm.coef[:, -1], r3.coef[:, 0])
        # the same candidates in reversed order; as a prefix of a longer batch whose extra rows cannot win
        rev = _lib.Candidates(ctx, Xc[::-1].copy())
        rr = _run(g, 0.01, eta, rev, 3, z)
        rev.close()
        np.testing.assert_array_equal(rr.indices, Xc.shape[0] - 1 - r3.indices)
        assert _bits(rr.acq[:, ::-1], r3.acq) and _bits(rr.coef[:, :, ::-1], r3.coef)
        longer = _lib.Candidates(ctx, np.vstack([Xc, og.X[:50]]))             # (training points: variance at noise level)
        rl = _run(g, 0.01, eta, longer, 3, z)
        longer.close()
        np.testing.assert_array_equal(rl.indices, r3.indices)
        assert _bits(rl.acq[:, :Xc.shape[0]], r3.acq) and rl.acq[:, Xc.shape[0]:].max() < r3.gains.min()
    finally:
        cand.close()
        g.close()
        g2.close()


def test_one_pass_equals_several_passes(ctx):
    N, D, M = 150, 3, 700
    rs, og, g, eta, Xc = TB._setup(ctx, dict(N=N, D=D, M=M))
    z = _z(16, 3, 2)
    try:
        ctx.set_tuning("ws_bytes", None)
        c1 = _lib.Candidates(ctx, Xc)
        r1 = _run(g, 0.0, eta, c1, 3, z)
        c1.close()
        ctx.set_tuning("ws_bytes", 128 * ((N + 1 + 127) // 128 * 128) * 8)      # a one-block workspace
        c2 = _lib.Candidates(ctx, Xc)
        r2 = _run(g, 0.0, eta, c2, 3, z)
        assert c2.chunk() == 128 and c2.chunk() < M
        c2.close()
    finally:
        ctx.set_tuning("ws_bytes", None)
        g.close()
    for name in ("indices", "gains", "flags", "acq", "trace", "coef", "d", "best"):
        assert _bits(getattr(r1, name), getattr(r2, name)), name


# ---- edges -------------------------------------------------------------------------------------------------------------------
EDGES = [dict(N=1, D=1, M=1, K=1, q=1, kernel="matern52"),
         dict(N=127, D=16, M=63, K=63, q=2, kernel="rbf"),
         dict(N=128, D=17, M=64, K=64, q=5, kernel="matern52", transform=(3.0, 2.5), par=0.02),
         # (length scales of 0.17: with the default ones and this noise the posterior has collapsed everywhere and one point wins
         # every pick, so the oracle's d_t could not stay above D_MIN)
         dict(N=129, D=3, M=65, K=65, q=5, kernel="fabolas", noise=1e-6, ls2=0.03),
         dict(N=257, D=2, M=401, K=1024, q=2, kernel="matern52"),
         # 64 picks: length scales of 0.03 keep the picks apart and every d_t well above the rounding of the residuals
         dict(N=40, D=2, M=300, K=4, q=64, kernel="matern52", ls2=1e-3, against_oracle=False)]


@pytest.mark.parametrize("e", EDGES, ids=lambda e: "N%d-D%d-m%d-K%d-q%d-%s" % (e["N"], e["D"], e["M"], e["K"], e["q"], e["kernel"]))
def test_edges_shapes(ctx, e):
    noise, transform, par = e.get("noise", 1e-2), e.get("transform", (0.0, 1.0)), e.get("par", 0.0)
    rs, X, y = TB._data(e["N"], e["D"], e.get("seed", 2))
    og, g = TB._pair(ctx, e["kernel"], TB._theta(e["D"], e.get("ls2", TB._ls2(e["D"])), noise, e["kernel"]), X, y, *transform)
    eta, Xc = float(y.min() * transform[1] + transform[0]), rs.rand(e["M"], e["D"])
    cand = _lib.Candidates(ctx, Xc)
    z = _z(e["K"], e["q"], 8)
    try:
        r = _run(g, par, eta, cand, e["q"], z)
        assert r.n_made == e["q"]
        if e.get("against_oracle", True):
            tol = (TB.BATCH_MU_ATOL, TB.BATCH_VAR_ATOL_REL_AMP) if noise >= 1e-3 else \
                (TB.BATCH_MU_ATOL_NOISE_1E8, TB.BATCH_VAR_ATOL_REL_AMP_NOISE_1E8)
            _check_each_pick(r, [og], Xc, z, par, eta, tol[0], tol[1], "edge")
        else:
            # 63 conditioning steps: the propagated bound of check 1 says nothing at that depth, so c_t(x), d_t and the
            # residual variances of every pick are held to the oracle's by a measured absolute bound (Q64_REL_AMP)
            _check_values_and_decisions(r, z, [og.y_std], "q = 64")
            assert len(set(r.indices)) == e["q"] and np.all(np.isfinite(r.gains))
            post = QO.JointPosterior(og, Xc)
            _, l, d, _ = post.condition([int(i) for i in r.indices[:-1]])
            amp = float(post.amp.max())
            assert np.all(d.astype(np.float64) >= D_MIN * amp)
            dc = np.abs(r.coef[:, 0] - (l * np.sqrt(d)[:, None]).astype(np.float64)).max() / amp
            dd = np.abs(r.d[:-1, 0] - d.astype(np.float64)).max() / amp
            var = post.var[None, :] - np.vstack([np.zeros((1, l.shape[1]), QO.LD), np.cumsum(l * l, axis=0)])
            dv = np.abs(r.trace[:, 0, :, 1] - post.var_t(var).astype(np.float64)).max() / (amp * og.y_std ** 2)
            dm = np.abs(r.trace[:, 0, :, 0] - post.mean_t.astype(np.float64)[None, :]).max()
            print("q = 64: max |dc| / k %.2e, |dd| / k %.2e, |dvar| / k %.2e, |dmu| %.2e" % (dc, dd, dv, dm))
            assert max(dc, dd, dv) <= Q64_REL_AMP and dm <= TB.BATCH_MU_ATOL
    finally:
        cand.close()
        g.close()


def test_edges_duplicates_nan_zero_z_and_refusals(ctx):
    sz = dict(N=80, D=3, M=120)
    rs, og, g, eta, Xc = TB._setup(ctx, sz, seed=4)
    z = _z(32, 3, 6)
    cand = _lib.Candidates(ctx, Xc)
    try:
        first = _run(g, 0.0, eta, cand, 3, z)
        p0 = int(first.indices[0])
        dup = 119 if p0 != 119 else 118
        Xd = Xc.copy()
        Xd[dup] = Xd[p0]                 # a duplicated row: the first index wins; then a candidate identical to an earlier pick
        lo, hi = min(p0, dup), max(p0, dup)
        cd = _lib.Candidates(ctx, Xd)
        r = _run(g, 0.0, eta, cd, 3, z)
        cd.close()
        assert r.indices[0] == lo and _bits(r.acq[0, lo], r.acq[0, hi])
        assert r.trace[1, 0, hi, 1] <= max(EPS, 4 * TB.BATCH_VAR_ATOL_REL_AMP * np.exp(og.theta[0]))     # its residual is gone
        assert _bits(r.acq[1, lo], r.acq[1, hi]) and _bits(r.coef[0, 0, lo], r.coef[0, 0, hi])
        _check_each_pick(r, [og], Xd, z, 0.0, eta, TB.BATCH_MU_ATOL, TB.BATCH_VAR_ATOL_REL_AMP, "duplicate")
        # z all zero: every scenario is the mean scenario
        r0 = _run(g, 0.0, eta, cand, 3, np.zeros((32, 3)))
        _check_each_pick(r0, [og], Xc, np.zeros((32, 3)), 0.0, eta, TB.BATCH_MU_ATOL, TB.BATCH_VAR_ATOL_REL_AMP, "z = 0")
        assert np.all(r0.best[1, 0] == r0.best[1, 0, 0])
        # a NaN candidate is np.argmax's winner: recorded, and ends the selection
        Xn = Xc[:40].copy()
        Xn[17, 1] = np.nan
        few = _lib.Candidates(ctx, Xn)
        rn = _run(g, 0.0, eta, few, 3, z)
        few.close()
        assert rn.n_made == 1 and rn.indices[0] == 17 and np.isnan(rn.gains[0]) and rn.flags[0] & _lib.FLAG_NAN
        np.testing.assert_array_equal(rn.indices[1:], [-1, -1])
        assert np.all(np.isnan(rn.gains[1:])) and np.all(np.isnan(rn.acq[1:])) and np.all(np.isnan(rn.best[1:]))
        # refusals
        for q in (0, -1, sz["M"] + 1):
            with pytest.raises(ValueError):
                g.select_batch_joint(0.0, eta, cand, q, _z(4, max(q, 1)))
        big = _lib.Candidates(ctx, rs.rand(70, 3))
        with pytest.raises(ValueError, match="q = 65"):
            g.select_batch_joint(0.0, eta, big, 65, _z(4, 65))
        big.close()
        with pytest.raises(ValueError, match="K = 1025"):
            g.select_batch_joint(0.0, eta, cand, 2, _z(1025, 2))
        with pytest.raises(ValueError):
            g.select_batch_joint(0.0, eta, cand, 2, np.zeros((0, 2)))
        with pytest.raises(ValueError, match="required"):
            g.select_batch_joint(0.0, eta, cand, 2, None)
        for bad in (np.nan, np.inf):
            zb = _z(8, 2)
            zb[5, 1] = bad
            with pytest.raises(ValueError, match="not finite"):
                g.select_batch_joint(0.0, eta, cand, 2, zb)
            with pytest.raises(ValueError, match="not finite"):                  # q = 1 does not use z; it is validated
                g.select_batch_joint(0.0, eta, cand, 1, zb[:, 1:])
        with pytest.raises(ValueError):
            g.select_batch_joint(0.0, eta, cand, 2, _z(8, 3))                     # the shape of z
        unfitted = _lib.DeviceGP(ctx, "matern52", 80, 3)
        unfitted.set_data(og.X, og.y)
        with pytest.raises(ValueError, match="trained"):
            unfitted.select_batch_joint(0.0, eta, cand, 2, _z(8, 2))
        unfitted.close()
        other = TB._setup(ctx, dict(N=80, D=2, M=5), seed=4)[2]                  # what ensemble_check refuses: another dimension
        with pytest.raises(ValueError):
            _lib.qei_batch([g, other], 0.0, eta, cand, 2, _z(8, 2))
        other.close()
        g.set_precision(1)
        g.fit(og.theta, og.mean)
        with pytest.raises(ValueError, match="fp64"):
            g.select_batch_joint(0.0, eta, cand, 2, _z(8, 2))
    finally:
        cand.close()
        g.close()


# ---- interpreter schedules ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"HIPEMU_GUARD": "1", "HIPEMU_ORDER": "1"}, {"HIPEMU_ORDER": "2"}],
                         ids=["fenced+descending", "rotating"])
def test_device_checks_fenced_and_in_any_work_item_order(env):
    """the interpreter's device checks again with every device buffer fenced by inaccessible pages and the work-items of a
    workgroup run in descending order, and once in rotating order"""
    import subprocess
    e = dict(os.environ, ROBO_TESTS_SERIAL="1", **env)
    e["PYTHONPATH"] = os.pathsep.join([os.path.dirname(HERE), e.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-p", "no:cacheprovider", "-m",
                        "not gpu", "-k", "every_pick or marginal or identities or passes or edges"], env=e,
                       cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout


# ---- classes and front end ---------------------------------------------------------------------------------------------------
def _model(rs, n=12):
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models import GaussianProcess
    lo, hi = TB._BOX
    X = lo + (hi - lo) * rs.rand(n, 2)
    y = np.array([TB._branin(x) for x in X]) / 50.0       # (targets of the prior's scale: a batch has somewhere else to go)
    model = GaussianProcess(Matern52Kernel(np.array([0.5, 0.5]), ndim=2), noise=1e-3, lower=lo, upper=hi)
    model.train(X, y, do_optimize=False)
    return model, X, y


def test_classes(ctx):
    from robo_amd.acquisition_functions import EI, LCB, PI, LogEI
    from robo_amd.maximizers import RandomSampling
    lo, hi = TB._BOX
    rs = np.random.RandomState(0)
    model, X, y = _model(rs)
    Xc = lo + (hi - lo) * rs.rand(100, 2)
    acq = EI(model)
    acq.update(model)
    pts = acq.select_batch(Xc, 3, fantasy="joint", n_mc=32, rng=np.random.RandomState(5), diagnostics=True)
    got = acq.last_batch
    assert pts.shape == (3, 2) and got.n_made == 3 and len(set(got.indices)) == 3
    np.testing.assert_allclose(pts, Xc[got.indices], rtol=0, atol=1e-12)
    # replayed from the seed: the same base samples through the library and through the oracle's fold
    z = np.random.RandomState(5).standard_normal((32, 3))
    cand = _lib.Candidates(model.gp.ctx, (Xc - lo) / (hi - lo))
    want = model.gp.select_batch_joint(acq.par, acq._eta(None), cand, 3, z, diagnostics=True)
    cand.close()
    for name in ("indices", "gains", "acq", "best"):
        assert _bits(getattr(got, name), getattr(want, name)), name
    _check_each_pick(got, [_frozen(model)], (Xc - lo) / (hi - lo), z, acq.par, acq._eta(None), TB.BATCH_MU_ATOL,
                     TB.BATCH_VAR_ATOL_REL_AMP, "EI class")
    np.testing.assert_array_equal(got.qei, np.cumsum(got.gains))
    again = acq.select_batch(Xc, 3, fantasy="joint", z=z)                     # z given: no draw
    np.testing.assert_array_equal(again, pts)
    for cls in (LogEI, PI, LCB):
        a = cls(model)
        a.update(model)
        with pytest.raises(TypeError, match="EI"):
            a.select_batch(Xc, 3, fantasy="joint")
    # defaults are today's results
    one = acq.select_batch(Xc, 3)
    assert isinstance(acq.last_batch, _lib.BatchResult) and one.shape == (3, 2)
    rsamp = RandomSampling(acq, lo, hi, n_samples=100, rng=np.random.RandomState(3))
    np.random.seed(5)
    P = rsamp.maximize_batch(3, fantasy="joint", n_mc=16)
    assert P.shape == (3, 2) and isinstance(acq.last_batch, _lib.QEIResult) and acq.last_batch.best is None
    np.random.seed(5)
    pool = rsamp.candidates()
    zz = np.random.RandomState(3).standard_normal((16, 3))
    np.testing.assert_array_equal(P, acq.select_batch(pool, 3, fantasy="joint", z=zz))


def _frozen(model):
    """the oracle's view of a trained robo_amd GaussianProcess: normalised inputs, latent targets, the fitted theta"""
    out = (float(model.y_mean), float(model.y_std)) if getattr(model, "normalize_output", False) else (0.0, 1.0)
    theta = np.concatenate([model.kernel.fixed_head(), model._fitted_theta])       # (a kernel without an amplitude factor: log amp 0)
    return TB.BO.FrozenGP(model.kernel.kind, theta, model.X, model.y, float(model.mean), *out)


def _y_std(model):
    return float(model.y_std) if getattr(model, "normalize_output", False) else 1.0


def test_marginalised_class(ctx):
    from robo_amd.acquisition_functions import EI, LogEI
    from robo_amd.acquisition_functions.marginalization import MarginalizationGPMCMC
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models.gaussian_process_mcmc import GaussianProcessMCMC
    from robo_amd.priors.default_priors import DefaultPrior
    lo, hi = TB._BOX
    rs = np.random.RandomState(2)
    X = lo + (hi - lo) * rs.rand(14, 2)
    y = np.array([TB._branin(x) for x in X]) / 50.0
    kernel = 2 * Matern52Kernel(np.ones(2), ndim=2)
    model = GaussianProcessMCMC(kernel, prior=DefaultPrior(len(kernel) + 1, rng=np.random.RandomState(3)), n_hypers=8,
                                chain_length=6, burnin_steps=4, rng=np.random.RandomState(4), lower=lo, upper=hi)
    model.train(X, y)
    acq = MarginalizationGPMCMC(EI(model))
    acq.update(model)
    Xc = lo + (hi - lo) * rs.rand(120, 2)
    pts = acq.select_batch(Xc, 3, fantasy="joint", n_mc=16, rng=np.random.RandomState(8), diagnostics=True)
    got = acq.last_batch
    z = np.random.RandomState(8).standard_normal((16, 3))
    gps = [e.model.gp for e in acq.estimators]
    etas = np.array([e._eta(None) for e in acq.estimators])
    cand = _lib.Candidates(gps[0].ctx, (Xc - lo) / (hi - lo))
    want = _lib.qei_batch(gps, acq.estimators[0].par, etas, cand, 3, z)
    cand.close()
    assert got.n_made == 3 and pts.shape == (3, 2) and got.trace.shape[1] == len(gps)
    assert _bits(got.indices, want.indices) and _bits(got.gains, want.gains)
    _check_each_pick(got, [_frozen(e.model) for e in acq.estimators], (Xc - lo) / (hi - lo), z, acq.estimators[0].par, etas,
                     TB.BATCH_MU_ATOL, TB.BATCH_VAR_ATOL_REL_AMP, "marginalised class")
    with pytest.raises(TypeError, match="EI"):
        MarginalizationGPMCMC(LogEI(model)).select_batch(Xc, 3, fantasy="joint")


def test_front_end(ctx):
    from robo_amd.fmin import bayesian_optimization
    res, calls = TB._bo(9, batch_size=3, fantasy="joint", n_mc=16)              # 3 initial points + two rounds of 3
    assert len(calls) == 9 and np.shape(res["X"]) == (9, 2)
    for rnd in (res["X"][3:6], res["X"][6:9]):
        assert len({tuple(x) for x in rnd}) == 3                                # distinct proposals
    a, _ = TB._bo(6)
    b, _ = TB._bo(6, n_mc=64)                                                   # the defaults are today's loop
    for key in a:
        if key not in ("runtime", "overhead"):
            np.testing.assert_array_equal(np.asarray(a[key]), np.asarray(b[key]), err_msg=key)
    seen = []
    for name in ("log_ei", "pi", "lcb"):
        with pytest.raises(ValueError, match="joint"):
            bayesian_optimization(lambda x: seen.append(x) or 0.0, TB._BOX[0], TB._BOX[1], num_iterations=6, maximizer="random",
                                  acquisition_func=name, model_type="gp", batch_size=3, fantasy="joint")
    assert not seen                                                             # before anything is evaluated


# ---- one larger case (MI355X) ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_larger_case_gpu():
    _lib.use_library(None)
    if _lib.device_count() < 1:
        pytest.skip("no HIP device")
    c = _lib.default_context()
    sz = dict(N=1100, D=16, M=32773, q=4, K=128)
    rs, og, g, eta, Xc = TB._setup(c, sz, seed=0)
    cand = _lib.Candidates(c, Xc)
    z = _z(sz["K"], sz["q"], 3)
    try:
        r = _run(g, 0.0, eta, cand, sz["q"], z)
        assert r.n_made == sz["q"]
        rows = set(range(0, sz["M"], 128)) | {int(i) for i in r.indices}
        for j in range(sz["q"]):
            rows |= {int(i) for i in np.argsort(r.acq[j])[-64:]}
        rows = np.array(sorted(rows))
        print("tiles: conditioning and fold grid %d workgroups of 64 candidates, %d tiles of 128 training rows, %d scenarios "
              "in 4 groups of %d" % ((sz["M"] + 63) // 64, (sz["N"] + 127) // 128, sz["K"], (sz["K"] + 3) // 4))
        left, total = _check_each_pick(r, [og], Xc, z, 0.0, eta, TB.BATCH_MU_ATOL_GPU, TB.BATCH_VAR_ATOL_REL_AMP_GPU,
                                       "gpu N = 1100", dtype=np.float64, rows=rows)
        assert 5 * left <= total
        # checks 2 and 3 on the same rows: the values from the device's own outputs, the argmax over ALL candidates
        sub = _lib.QEIResult(r.indices, r.gains, r.flags, r.n_made, r.acq[:, rows], r.trace[:, :, rows], r.coef[:, :, rows],
                             r.d, r.best)
        for j in range(sz["q"]):
            want = _device_values(sub, j, z, [og.y_std]).astype(np.float64)
            np.testing.assert_allclose(sub.acq[j], want, rtol=ACQ_RTOL + sz["K"] * EPS, atol=0)
            assert int(r.indices[j]) == O.np_argmax(r.acq[j]) and _bits(r.gains[j], r.acq[j, int(r.indices[j])])
    finally:
        cand.close()
        g.close()
