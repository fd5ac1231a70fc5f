"""The gradient of the log marginal likelihood (robo_gp_grad_loglik, robo_gp_grad_loglik_batch: csrc/gradient.hip driven from
api_fit.hip and hyperopt.hip) against the extended-precision oracle (tests/cov_oracle.py Posterior.grad_loglik) at the edges of
its five stages:

  * triinv_base / triinv_kernel<TM>: W = L^-1 by pairwise merges of 128-blocks (N one off a block, 5 / 7 / 9 block rows:
    the second half of a merge pair clipped to 1 or 3 blocks; both TM)                                          -- G1, G4
  * alpha_kernel (reads z out of the augmented row: the mean offset must show)                                      -- G1
  * kinv_tile_kernel: A = alpha alpha^T - W^T W on 128 x 128 tiles                                                  -- G1
  * grad_reduce_kernel<KIND>: 64 x 64 tiles (N = 63, 64, 65), dimensions staged 16 at a time (D = 15, 16, 17, 32, 33,
    MAX_DIM; Fabolas: the fidelity column first in, or alone in, a pass), the scalar slots                         -- G2, G3
  * grad_final_kernel                                                                                              -- all
  * one handle over several n, shared workspaces (d_gV with the explicit inverse), the kept batch workspace         -- G5

The functions take a context and run in two settings (tests/test_loglik_gradient.py), as those of vcons_checks.py do: the
interpreted build of the sources on the CPU and librobo_hip.so on an MI355X.

Inputs are drawn as vcons_checks.Case draws them: X uniform in [0, 1]^D, y = sin(3 sum x) + 0.1 noise, theta = [ln amp,
ln metric ..., (ln a, ln b,) ln noise] with amp 1.3, noise 3e-3, Fabolas a = 0.8, b = 1.3, unequal metrics around
1 / (0.4 d_in); rows scaled with cov_oracle.scale; mean_c = mean(y), and mean(y) + 0.37 in the N = 257 case of each kind.
With that draw the scaled distances grow like d_in: from D = 32 on the off-diagonal covariances are below 1e-8 of the
amplitude and at D = 256 they underflow, which leaves the metric entries of those cases next to nothing to be wrong about.  G2
therefore runs every D >= 15 a second time with the metrics around 0.4 d_in (`smooth`: squared scaled distances around
1 / 2.4, strongly correlated rows), an addition to the stated cases, under the same bound.

Tolerances -- none is tuned on the code under test.  Per case, with g the long-double oracle, S_p = 1/2 sum_ij |A_ij dK_ij /
d theta_p| the magnitude the p-th sum is conditioned by, and `dev` the largest deviation over the P entries of the same
algorithm in np.float64 (Posterior(dtype=np.float64)) from the long-double oracle:
  * every entry:  |device - g|_p <= 1e-13 max_p S_p + 20 dev -- 1e-13 is cov_checks' C2 entry tolerance, 20 the head-room
    check_feeds uses between the blocked algorithm and the straightforward fp64 one;
  * additionally every entry stays under the present contract (parity_checks.check_grad_loglik): rtol 1e-8, atol 1e-9 of the
    largest entry;
  * log-likelihood:  LOGLIK_RTOL |ll| + 20 dev_ll, as in check_feeds;
  * bit-for-bit claims (batch == single, TM = 4 == TM = 1, reuse == fresh handle, exact zero of a constant column's entry) are
    asserted as such.
Every check prints its worst error / tolerance before it asserts; NOTES.md "likelihood gradient checks" records the measured
ones."""
import numpy as np

import cov_oracle as CO
from _tol import LOGLIK_RTOL
from cov_checks import _report, gram_needs_direct
from robo_amd import _lib
from vcons_checks import bits, n_pad_of

L = np.longdouble
ENTRY_REL = 1e-13                                # cov_checks C2
HEADROOM = 20.0                                  # cov_checks.check_feeds
CONTRACT_RTOL, CONTRACT_ATOL_REL = 1e-8, 1e-9    # parity_checks.check_grad_loglik
MEAN_OFFSET = 0.37
WS_DEFAULT = 6 << 30                             # csrc/common.h: the default workspace (ws_bytes)


def sample_bytes(N, D, P):
    """what one sample takes of ws_bytes in robo_gp_grad_loglik_batch (hyperopt.hip hyper_sample_bytes)"""
    npad = n_pad_of(N)
    t64 = (N + 63) // 64
    return 8 * (3 * npad * npad + npad * (128 + D) + npad + P * (t64 * (t64 + 1) // 2) + P)


# ---- cases: inputs and their oracle, once per process ---------------------------------------------------------------------------
class Case(object):
    """one data set and its thetas: theta 0 as vcons_checks.Case draws it, thetas 1 .. 3 around it (all entries moved by
    0.15 randn).  oracle(i): the long-double gradient at theta i and the deviation of its fp64 twin, computed once."""

    def __init__(self, kind, N, D, mean_offset=0.0, smooth=False, special=False, seed=0):
        rs = np.random.RandomState(100000 * seed + 100 * N + D)
        fab = kind == "fabolas"
        d_in = D - 1 if fab else D
        self.key = (kind, N, D, mean_offset, smooth, special, seed)
        self.kind, self.N, self.D, self.d_in, self.fab = kind, N, D, d_in, fab
        self.X = rs.rand(N, D)
        if special:
            assert N >= 100 and d_in >= 3
            self.X[77] = self.X[5]                   # r2 = 0 off the diagonal, across a 64-tile boundary
            self.X[40, 0] = 1e4                      # every covariance with row 40 underflows to 0 (oracle: below 1e-4951)
            self.X[:, 1] = 0.37                      # a constant column: d K / d ln m_1 = 0 exactly
            if fab:
                self.X[3, -1], self.X[9, -1] = 0.0, 1.0
        self.y = np.sin(3.0 * self.X.sum(axis=1)) + 0.1 * rs.randn(N)
        self.mean = float(self.y.mean()) + mean_offset
        lnm = (np.log(0.4 * d_in) if smooth else -np.log(0.4 * d_in)) + 0.3 * rs.randn(d_in)
        head = [np.log(1.3)]
        tail = [np.log(0.8), np.log(1.3), np.log(3e-3)] if fab else [np.log(3e-3)]
        theta0 = np.concatenate([head, lnm, tail])
        self.thetas = np.vstack([theta0[None, :], theta0[None, :] + 0.15 * rs.randn(3, theta0.size)])
        self.P = theta0.size
        self._oracle = {}

    def parts(self, theta):
        """what the device reads out of theta -> (amp, noise, (a, b), scaled rows)"""
        theta = np.asarray(theta, dtype=np.float64)
        amp, noise = float(np.exp(theta[0])), float(np.exp(theta[-1]))
        blr = (float(np.exp(theta[-3])), float(np.exp(theta[-2]))) if self.fab else (1.0, 1.0)
        return amp, noise, blr, CO.scale(self.X, theta[1:1 + self.d_in], n_scaled=self.d_in)

    def oracle_at(self, theta):
        amp, noise, blr, Xs = self.parts(theta)
        o = CO.Posterior(self.kind, amp, noise, Xs, self.y, self.mean, blr=blr)
        t = CO.Posterior(self.kind, amp, noise, Xs, self.y, self.mean, blr=blr, dtype=np.float64)
        (g, S), (g64, _) = o.grad_loglik(), t.grad_loglik()
        assert g.dtype == L and g64.dtype == np.float64 and g.shape == (self.P,)
        return dict(g=g, S=S, ll=o.loglik, dev=float(np.max(np.abs(g64 - g))), dev_ll=abs(float(t.loglik - o.loglik)),
                    dev_rel=float(np.max(np.abs(g64 - g)) / np.max(np.abs(g))))

    def oracle(self, i=0):
        if i not in self._oracle:
            self._oracle[i] = self.oracle_at(self.thetas[i])
        return self._oracle[i]


_CASES = {}


def case(kind, N, D, mean_offset=0.0, smooth=False, special=False, seed=0):
    key = (kind, N, D, mean_offset, smooth, special, seed)
    if key not in _CASES:
        _CASES[key] = Case(*key)
    return _CASES[key]


def _finish(worst):
    bad = [msg for r, msg in worst if not r <= 1.0]
    assert not bad, bad
    return max(r for r, _ in worst)


def against_oracle(label, c, o, ll, grad):
    """one (ll, gradient) of the device against the oracle `o` of the same theta -> [(ratio, message), ...]"""
    assert np.isfinite(ll) and np.all(np.isfinite(grad)) and grad.shape == (c.P,), (label, ll, grad)
    tol = ENTRY_REL * float(np.max(o["S"])) + HEADROOM * o["dev"]
    err = np.abs(grad - o["g"]).astype(np.float64)
    go = np.abs(o["g"]).astype(np.float64)
    out = [_report(label + " gradient (fp64 twin deviates %.3g relative)" % o["dev_rel"], err, np.full(c.P, tol)),
           _report(label + " gradient, rtol 1e-8 / atol 1e-9 contract", err, CONTRACT_RTOL * go + CONTRACT_ATOL_REL * go.max())]
    ll_o = float(o["ll"])
    out.append(_report(label + " loglik", np.array([abs(ll - ll_o)]), np.array([LOGLIK_RTOL * abs(ll_o) + HEADROOM * o["dev_ll"]])))
    return out


def handle(ctx, c, n_max=None):
    g = _lib.DeviceGP(ctx, c.kind, c.N if n_max is None else n_max, c.D)
    g.set_data(c.X, c.y)
    return g


# ---- G1, G2 (+ G4 ordinary batches): shapes ---------------------------------------------------------------------------------------
G1_N = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 512, 513, 640, 641)
G1_N_GPU = (770, 1024, 1025)                     # 7, 8, 9 block rows; n_pad 896 / 1152 / 1152
G1_N_OTHER = (64, 128, 129, 257, 385, 513)


def _offset(N):
    return MEAN_OFFSET if N == 257 else 0.0


G1_CASES = tuple(("matern52", N, 3, _offset(N), False) for N in G1_N) + \
    tuple((kind, N, 4, _offset(N), False) for kind in ("rbf", "fabolas") for N in G1_N_OTHER)
G1_CASES_GPU = tuple(("matern52", N, 3, 0.0, False) for N in G1_N_GPU)
# N = 641 takes 17 s through the interpreter (640: 12 s): there 640 stays and 641 runs on the GPU only
G1_CASES_EMU = tuple(c for c in G1_CASES if c[1] != 641)
G2_D = {"matern52": (1, 15, 16, 17, 32, 33, 256), "rbf": (1, 15, 16, 17, 32, 33, 256), "fabolas": (2, 16, 17, 18, 33, 256)}
G2_CASES = tuple((kind, N, D, 0.0, smooth) for kind in ("matern52", "rbf", "fabolas") for N in (65, 129) for D in G2_D[kind]
                 for smooth in ((False, True) if D >= 15 else (False,)))


def check_shape(ctx, kind, N, D, mean_offset=0.0, smooth=False):
    """G1 / G2 for one shape, and G4's ordinary batch on it.  grad_loglik at theta 0 against the oracle; the call repeated:
    the same bits; grad_loglik_batch of thetas 0 .. 2 equals the three single calls bit for bit, ll and gradient (the single
    calls run AFTER the batch on the same handle, so the batch cannot have borrowed anything from them)."""
    c = case(kind, N, D, mean_offset, smooth)
    o = c.oracle()
    label = "%s N=%d D=%d%s%s" % (kind, N, D, " smooth" if smooth else "", " mean+%.2f" % mean_offset if mean_offset else "")
    g = handle(ctx, c)
    try:
        llb, gb, st = g.grad_loglik_batch(c.thetas[:3], c.mean)
        assert np.all(st == _lib.OK), (label, st)
        ll, grad = g.grad_loglik(c.thetas[0], c.mean)
        worst = against_oracle(label, c, o, ll, grad)
        if mean_offset:
            # the offset shows: the ORACLE of the same data at mean(y) is at least 1e4 tolerances away in some entry, so a
            # kernel that read y - mean(y) from anywhere but the augmented row would miss the bound by that much
            plain = case(kind, N, D, 0.0, smooth).oracle()
            tol = ENTRY_REL * float(np.max(o["S"])) + HEADROOM * o["dev"]
            assert float(np.max(np.abs(plain["g"] - o["g"]))) > 1e4 * tol, (label, plain["g"], o["g"], tol)
        ll2, grad2 = g.grad_loglik(c.thetas[0], c.mean)
        assert ll2 == ll and bits(grad2, grad), label + ": not repeatable bit for bit"
        for s in range(3):
            ll1, g1 = (ll, grad) if s == 0 else g.grad_loglik(c.thetas[s], c.mean)
            assert llb[s] == ll1, "%s: batch sample %d loglik %r != single %r" % (label, s, llb[s], ll1)
            assert bits(gb[s], g1), "%s: batch sample %d gradient differs from the single call by %.3g" % (
                label, s, float(np.max(np.abs(gb[s] - g1))))
    finally:
        g.close()
    return _finish(worst)


# ---- G3: special pairs --------------------------------------------------------------------------------------------------------
G3_CASES = (("matern52", 130, 3), ("rbf", 130, 4), ("fabolas", 130, 4))


def check_special(ctx, kind, N, D):
    """G3.  One data set per kind: rows 5 and 77 identical (r2 = 0 off the diagonal, in another 64-row tile); row 40 moved to
    x_0 = 1e4 so that every covariance with it is 0 (exp(-t) times the growing Matern polynomial or times diff^2: 0, not
    inf x 0); column 1 constant, for which the device's entry is exactly +-0.0 (every term is e_ij x 0); Fabolas: fidelity
    values exactly 0 (B = a: the ln b term vanishes) and exactly 1 present.  The batch of thetas 0 .. 2 equals the single calls
    bit for bit here too, the exact zero included."""
    c = case(kind, N, D, special=True)
    o = c.oracle()
    amp, _, blr, Xs = c.parts(c.thetas[0])
    K = CO.kernel(kind, amp, Xs, blr=blr)
    assert np.all(np.delete(K[40], 40) == 0) and K[5, 77] == K[5, 5] and float(o["g"][2]) == 0.0
    label = "G3 %s N=%d D=%d" % (kind, N, D)
    g = handle(ctx, c)
    try:
        ll, grad = g.grad_loglik(c.thetas[0], c.mean)
        worst = against_oracle(label, c, o, ll, grad)
        assert grad[2] == 0.0, "%s: the constant column's metric entry is %r" % (label, grad[2])
        llb, gb, st = g.grad_loglik_batch(c.thetas[:3], c.mean)
        assert np.all(st == _lib.OK) and np.all(gb[:, 2] == 0.0), (label, st, gb[:, 2])
        for s in range(3):
            ll1, g1 = (ll, grad) if s == 0 else g.grad_loglik(c.thetas[s], c.mean)
            assert llb[s] == ll1 and bits(gb[s], g1), "%s: batch sample %d differs from the single call" % (label, s)
    finally:
        g.close()
    return _finish(worst)


# ---- G4: batch == single --------------------------------------------------------------------------------------------------------
MIXED = dict(kind="matern52", N=130, D=3, offset=10.0, lnm_direct=-8.0, lnm_dot=1.0)


def check_mixed_batch(ctx):
    """G4.  A batch in which ONE sample takes the direct-difference gram tile and two the dot form (fb.gram_mixed = any_direct
    switches the gram kernel of the whole group) equals the single calls bit for bit.  Data offset by +10, ln m = -8 for the
    direct sample against ln m around 1: cov_checks.gram_needs_direct -- the mirror of the library's criterion -- is asserted to
    say direct / dot / dot, each a factor two or more off the bound.  (Offset by +50 the criterion is 7.6e-12 > 1e-12 at
    ln m = 1 as well, and nothing would be mixed.)  The direct sample also meets the oracle."""
    m = MIXED
    c = case(m["kind"], m["N"], m["D"], seed=3)
    X = c.X + m["offset"]
    rs = np.random.RandomState(11)
    thetas = np.vstack([c.thetas[0]] * 3)
    thetas[0, 1:1 + c.D] = m["lnm_dot"] + 0.1 * rs.randn(c.D)
    thetas[1, 1:1 + c.D] = m["lnm_direct"]
    thetas[2, 1:1 + c.D] = m["lnm_dot"] + 0.1 * rs.randn(c.D)
    thetas[2, 0] += 0.2
    for s, want in enumerate((False, True, False)):
        lnm = thetas[s, 1:1 + c.D]
        assert gram_needs_direct(X, lnm) == want, (s, want)
        assert gram_needs_direct(X * np.sqrt(2.0), lnm) == want and gram_needs_direct(X / np.sqrt(2.0), lnm) == want, s
    g = _lib.DeviceGP(ctx, c.kind, c.N, c.D)
    try:
        g.set_data(X, c.y)
        llb, gb, st = g.grad_loglik_batch(thetas, c.mean)
        assert np.all(st == _lib.OK), st
        for s in range(3):
            ll1, g1 = g.grad_loglik(thetas[s], c.mean)
            assert llb[s] == ll1 and bits(gb[s], g1), "mixed batch: sample %d differs from the single call (%.3g)" % (
                s, float(np.max(np.abs(gb[s] - g1))))
        shifted = Case(c.kind, c.N, c.D, seed=3)
        shifted.X = X
        return _finish(against_oracle("G4 mixed batch, the direct sample", shifted, shifted.oracle_at(thetas[1]), llb[1], gb[1]))
    finally:
        g.close()


WIDE_N = (300, 520)                              # 3 and 5 block rows


def triinv_levels(N, S, num_cu):
    """gradient.hip launch_grad_loglik_batch restated: [(sb, pairs, narrow)] per level; narrow: triinv_batch_kernel<1> (32-row
    sub-tiles), otherwise <4>"""
    nbk = (N + 127) // 128
    out, sb = [], 1
    while sb < nbk:
        pairs = (nbk + 2 * sb - 1) // (2 * sb)
        out.append((sb, pairs, sb * sb * pairs * S <= 2 * num_cu))
        sb *= 2
    return out


def check_wide_batch(ctx, num_cu, N):
    """G4.  launch_grad_loglik_batch takes triinv_batch_kernel<4> at a level when sb^2 pairs S > 2 num_cu.  With nbk block rows the
    bottom level (sb = 1) has ceil(nbk / 2) pairs and is the last to leave TM = 1, so S1 = 2 num_cu // ceil(nbk / 2) + 1 is the
    smallest batch in which every level takes TM = 4, and S1 - 1 the last in which the bottom level still takes TM = 1 (257 /
    256 at N = 300 and 171 / 170 at N = 520 on the 256-CU part).  The interpreter reports one CU: S1 = 2 and 1, raised to 3.
    The samples cycle through the case's 4 thetas; every sample equals the single call of its theta bit for bit (on the
    device a single call takes TM = 1 at every level: asserted from the same rule with S = 1), and the 4 thetas meet the
    oracle.  The batch must go as ONE group of the default workspace: sample_bytes S is asserted to fit."""
    c = case("matern52", N, 3, seed=7)
    nbk = (N + 127) // 128
    s1_rule = 2 * num_cu // ((nbk + 1) // 2) + 1
    s1 = max(s1_rule, 3)
    g = handle(ctx, c)
    worst = []
    try:
        single = [g.grad_loglik(c.thetas[i], c.mean) for i in range(4)]
        for i, (ll, grad) in enumerate(single):
            worst += against_oracle("G4 wide N=%d theta %d" % (N, i), c, c.oracle(i), ll, grad)
        if num_cu > 4:
            assert all(narrow for _, _, narrow in triinv_levels(N, 1, num_cu)), (N, num_cu)     # the single call: TM = 1
        for S in (s1, s1 - 1):
            levels = triinv_levels(N, S, num_cu)
            print("G4 wide N=%d nbk=%d num_cu=%d S=%d: levels (sb, pairs, TM=1) %s" % (N, nbk, num_cu, S, levels))
            assert levels[0][:2] == (1, (nbk + 1) // 2), levels
            if S == s1:
                assert not any(narrow for _, _, narrow in levels), levels                      # TM = 4 at every level
            elif s1 == s1_rule:
                assert levels[0][2] and not any(narrow for _, _, narrow in levels[1:]), levels  # TM = 1 at the bottom only
            assert sample_bytes(N, c.D, c.P) * S <= WS_DEFAULT, (N, S)
            idx = np.arange(S) % 4
            llb, gb, st = g.grad_loglik_batch(c.thetas[idx], c.mean)
            assert np.all(st == _lib.OK), (N, S, st[st != _lib.OK][:4])
            for s in range(S):
                ll1, g1 = single[idx[s]]
                assert llb[s] == ll1 and bits(gb[s], g1), "G4 wide N=%d S=%d: sample %d (theta %d) differs from the single " \
                    "call by %.3g" % (N, S, s, idx[s], float(np.max(np.abs(gb[s] - g1))))
    finally:
        g.close()
    return _finish(worst)


# ---- G5: one handle, several n ------------------------------------------------------------------------------------------------
REUSE = dict(kind="matern52", D=3, n_max=400, ns=(385, 130, 250, 64, 257), winv_ns=(385, 257), m=5)


def check_reuse(ctx):
    """G5.  One handle of n_max = 400 (d_gV / d_gA / d_gpart sized for n_pad_max = 512) takes set_data + grad_loglik +
    grad_loglik_batch (S = 3) at n = 385, 130, 250, 64, 257 in turn: n_pad 512, 256, 256, 128, 384 -- 130 -> 250 keeps n_pad with
    a larger n (hyper_grad_ensure keeps its workspace, whose 64-row tiles are counted for n_pad), 64 follows a larger n in
    every buffer.  Each result is bitwise that of a fresh handle of exactly that n.  At n = 385 and 257, with the explicit
    inverse selected as parity_checks.check_winv_path selects it (winv_min_blocks = 2; 5 candidates: the matrix-vector form,
    whose build shares d_gV with the gradient): predict, grad_loglik at another theta, predict -- equal to the predict of a
    fresh handle fitted at that theta --, then fit at the first theta with no call between, predict -- equal to the first."""
    r = REUSE
    big = _lib.DeviceGP(ctx, r["kind"], r["n_max"], r["D"])
    rs = np.random.RandomState(17)
    Xc = rs.rand(r["m"], r["D"])
    try:
        ctx.set_tuning("winv_min_blocks", 2)
        for n in r["ns"]:
            c = case(r["kind"], n, r["D"], seed=5)
            t0, t1 = c.thetas[0], c.thetas[1]
            fresh = _lib.DeviceGP(ctx, r["kind"], n, r["D"])
            cand, cand_f = _lib.Candidates(ctx, Xc), _lib.Candidates(ctx, Xc)
            try:
                big.set_data(c.X, c.y)
                fresh.set_data(c.X, c.y)
                tag = "G5 n=%d" % n
                ll, grad = big.grad_loglik(t0, c.mean)
                ll_f, grad_f = fresh.grad_loglik(t0, c.mean)
                assert ll == ll_f and bits(grad, grad_f), "%s: grad_loglik differs from a fresh handle by %.3g" % (
                    tag, float(np.max(np.abs(grad - grad_f))))
                llb, gb, st = big.grad_loglik_batch(c.thetas[:3], c.mean)
                llb_f, gb_f, st_f = fresh.grad_loglik_batch(c.thetas[:3], c.mean)
                assert np.all(st == _lib.OK) and np.all(st_f == _lib.OK), tag
                assert bits(llb, llb_f) and bits(gb, gb_f), "%s: grad_loglik_batch differs from a fresh handle by %.3g" % (
                    tag, float(np.max(np.abs(gb - gb_f))))
                assert llb[0] == ll and bits(gb[0], grad), tag
                if n in r["winv_ns"]:
                    big.fit(t0, c.mean)
                    p0 = big.predict(cand)
                    assert cand.solve_kernel() == "winv_gemv_kernel", (tag, cand.solve_kernel())
                    big.grad_loglik(t1, c.mean)                                # leaves the handle fitted at t1; d_gV rewritten
                    p1 = big.predict(cand)
                    assert cand.solve_kernel() == "winv_gemv_kernel", (tag, cand.solve_kernel())
                    fresh.fit(t1, c.mean)
                    p1_f = fresh.predict(cand_f)
                    assert cand_f.solve_kernel() == "winv_gemv_kernel", (tag, cand_f.solve_kernel())
                    assert bits(p1[0], p1_f[0]) and bits(p1[1], p1_f[1]), tag + ": predict after grad_loglik at another theta"
                    assert not bits(p1[0], p0[0]), tag
                    big.fit(t0, c.mean)
                    p2 = big.predict(cand)
                    assert cand.solve_kernel() == "winv_gemv_kernel", (tag, cand.solve_kernel())
                    assert bits(p2[0], p0[0]) and bits(p2[1], p0[1]), tag + ": predict after the fit back at the first theta"
                print("%s: bitwise equal to a fresh handle" % tag)
            finally:
                cand.close()
                cand_f.close()
                fresh.close()
    finally:
        ctx.set_tuning("winv_min_blocks", None)
        big.close()
