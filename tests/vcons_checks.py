"""The entry points that consume V = L^-1 K*^T itself and not only its row reductions, against the extended-precision oracle
(tests/cov_oracle.py Posterior.covariance / Posterior.gradients) past one 128-row tile:

  * robo_gp_predict_cov  (cov_kernel, predict.hip: a (t, t) grid of 128 x 128 tiles)                                -- V1, V2
  * robo_gp_cross_cov    (cross_cov_kernel, infogain.hip: its 32-row and its 128-row tile; chunked workspaces)      -- V2, V3, V5
  * robo_ig_eval_cand    (gemm_nt_kernel, infogain.hip: the same two tiles)                                         -- V3, V5
  * robo_gp_predict_grad (predgrad.hip: D + 1 pseudo-rows per candidate, several passes)                            -- V4

The functions take a context and run in two settings (tests/test_v_consumers.py), as those of cov_checks.py do: the
interpreted build of the sources on the CPU and librobo_hip.so on an MI355X.

Inputs follow cov_checks.check_feeds: theta = [ln amp, ln metric ..., (ln a, ln b,) ln noise], rows scaled with
cov_oracle.scale; moderate conditioning (metrics around 1 / (0.4 D), unequal per dimension, noise 3e-3); D in {3, 4}; the
three kernels.  The oracle of a case is computed once per process and shared by both settings.

Tolerances -- none is tuned on the code under test.  With `dev` the largest deviation, over the compared array, of the same
algorithm in np.float64 (cov_oracle.Posterior(dtype=np.float64)) from the np.longdouble oracle, and `amp` the largest prior
variance k(x, x) of the case's points (the amplitude; Fabolas: amp (a + b u^2)):
  * covariance and cross-covariance entries:  (1e-13 amp + 20 dev) y_std^2 -- 1e-13 is cov_checks' C2 entry tolerance, 20 the
    head-room check_feeds uses between the blocked algorithm and the straightforward fp64 one; additionally every entry stays
    under the present contract, VAR_ATOL_REL_AMP amp y_std^2 (covariances) and 1e-9 amp (cross-covariances);
  * gradients:  1e-13 max |oracle array| + 20 dev, times y_std (mean) or y_std^2 (variance);
  * through the explicit inverse W (winv.hip): the same plus 3e-11 amp, the agreement parity_checks.check_winv_path grants W
    against the substitution;
  * bit-for-bit claims are asserted as such.
Every check prints its worst error / tolerance before it asserts; NOTES.md "V consumers" records the measured ones."""
import numpy as np

import cov_oracle as CO
from _tol import MU_ATOL, MU_RTOL, VAR_ATOL_REL_AMP
from cov_checks import _report
from oracle import ig_oracle as IG
from robo_amd import _lib
from robo_amd.util import epmgp

L = np.longdouble
EPS = 2.220446049250313e-16
TRANSFORMS = ((0.0, 1.0), (0.3, 2.5))            # (y_mean, y_std): the identity and a real one
ENTRY_REL_AMP = 1e-13                            # cov_checks C2
HEADROOM = 20.0                                  # cov_checks.check_feeds
WINV_REL_AMP = 3e-11                             # parity_checks.check_winv_path
CROSS_CONTRACT_REL_AMP = 1e-9                    # tests/test_infogain.py, parity_checks.check_winv_path
IG_RTOL = 1e-6                                   # tests/test_infogain.py _check_ig

STEP_SMALL, STEP_GEN, STEP_PAIR, STEPWISE, CHAIN = ("trsm_step_small_kernel", "trsm_step_gen_kernel", "trsm_pair_gen_kernel",
                                                    "trsm_step_kernel", "trsm_chain_kernel")
WINV_GEMV, WINV_GEMM, WINV_ROW = "winv_gemv_kernel", "winv_gemm_kernel", "winv_row_kernel"


def bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def n_pad_of(N):
    return (N + 1 + 127) // 128 * 128            # robo_amd/csrc/api_fit.hip: round_up(n + 1, 128)


# ---- cases: inputs and their oracle, once per process ---------------------------------------------------------------------------
class Case(object):
    """one data set, its candidates Xc (M rows) and reference points Z (nb rows), the long-double oracle and its fp64 twin"""

    def __init__(self, kind, N, D, M, nb=0, seed=0):
        rs = np.random.RandomState(100000 * seed + 100 * N + D)
        fab = kind == "fabolas"
        d_in = D - 1 if fab else D
        self.key = (kind, N, D, M, nb, seed)
        self.kind, self.N, self.D, self.M, self.nb = kind, N, D, M, nb
        self.X = rs.rand(N, D)
        self.y = np.sin(3.0 * self.X.sum(axis=1)) + 0.1 * rs.randn(N)
        self.mean = float(self.y.mean())
        self.lnm = -np.log(0.4 * d_in) + 0.3 * rs.randn(d_in)                  # unequal metrics around 1 / (0.4 D)
        head = [np.log(1.3)]
        tail = [np.log(0.8), np.log(1.3), np.log(3e-3)] if fab else [np.log(3e-3)]
        self.theta = np.concatenate([head, self.lnm, tail])
        # what the device reads out of theta
        self.amp, self.noise = float(np.exp(self.theta[0])), float(np.exp(self.theta[-1]))
        self.blr = (float(np.exp(self.theta[-3])), float(np.exp(self.theta[-2]))) if fab else (1.0, 1.0)
        self.Xc = rs.rand(M, D)
        self.Z = rs.rand(nb, D)
        if nb:
            # the last candidate sits next to the first reference point: the only live row of a ragged last tile (M = 129)
            # then has an entry well above the clip, which would otherwise hide what that row was computed from
            self.Xc[-1] = np.minimum(self.Z[0] + 0.02, 1.0)
        self.ism = CO.scale(np.ones((1, D)), self.lnm, n_scaled=d_in)[0]         # d xs_d / d x_d (1 on the fidelity column)
        self.Xs, self.Xcs, self.Zs = (CO.scale(A, self.lnm, n_scaled=d_in) for A in (self.X, self.Xc, self.Z))
        u2 = float(max(np.max(self.Xc[:, -1] ** 2), np.max(self.Z[:, -1] ** 2) if nb else 0.0))
        self.kscale = self.amp * (self.blr[0] + self.blr[1] * u2) if fab else self.amp
        self._memo = {}

    def posterior(self, dtype):
        return self.memo(("posterior", np.dtype(dtype).name),
                         lambda: CO.Posterior(self.kind, self.amp, self.noise, self.Xs, self.y, self.mean, blr=self.blr,
                                              dtype=dtype))

    def memo(self, name, fn):
        if name not in self._memo:
            self._memo[name] = fn()
        return self._memo[name]

    def both(self, name, fn):
        """fn(posterior) in long double and in fp64 -> (oracle, largest deviation of the fp64 twin per returned array)"""
        def run():
            o, t = fn(self.posterior(L)), fn(self.posterior(np.float64))
            if isinstance(o, tuple):
                return o, tuple(float(np.max(np.abs(a - b))) for a, b in zip(o, t)), t
            return o, float(np.max(np.abs(o - t))), t
        return self.memo(name, run)


_CASES, _FITTED = {}, {}


def case(kind, N, D, M, nb=0, seed=0):
    key = (kind, N, D, M, nb, seed)
    if key not in _CASES:
        _CASES[key] = Case(*key)
    return _CASES[key]


def fitted(ctx, c):
    """the fitted device GP of a case: once per (context, case); identity output transform"""
    key = (id(ctx), c.key)
    if key not in _FITTED:
        g = _lib.DeviceGP(ctx, c.kind, c.N, c.D)
        g.set_data(c.X, c.y)
        g.fit(c.theta, c.mean)
        _FITTED[key] = g
    return _FITTED[key]


def drop(ctx):
    for key in [k for k in _FITTED if k[0] == id(ctx)]:
        _FITTED.pop(key).close()


def producer(ctx, g, Xc):
    """the solve kernel a `predict` of these points takes on a Candidates handle under the present tuning.  robo_gp_predict_cov
    owns its handle, so for it this is a STAND-IN: the same points, the same tuning, the same decision (api_predict.hip
    predict_core with the chained form allowed), read where it can be read."""
    cand = _lib.Candidates(ctx, Xc)
    try:
        g.predict(cand)
        return cand.solve_kernel()
    finally:
        cand.close()


def entry_tol(c, dev, y_std, name=""):
    extra = WINV_REL_AMP * c.kscale if name.startswith("winv_") else 0.0
    return (ENTRY_REL_AMP * c.kscale + HEADROOM * dev + extra) * y_std * y_std


def _finish(worst):
    bad = [msg for r, msg in worst if not r <= 1.0]
    assert not bad, bad
    return max(r for r, _ in worst)


# ---- V1: the full covariance past one tile ------------------------------------------------------------------------------------
FULL_COV_CASES = (("rbf", 128, 4), ("fabolas", 256, 4), ("matern52", 257, 3))
FULL_COV_MS = (1, 128, 129, 257)


def check_full_cov(ctx, kind, N, D):
    """V1.  N = 128 / 256 / 257: one block row and the skipped trailing block, two and the skipped block, three ragged ones
    (chained by default); m = 1, 128, 129, 257: one tile, a full one, a ragged second, a ragged third, i.e. a (3, 3) grid with
    off-diagonal tiles; both output transforms.  Every entry against the oracle's signed covariance; C == C^T bit for bit;
    max(diag C, eps) against `predict`'s variance of the same points; the mean against the oracle's at check_feeds' bound.
    Under one producer family (winv_max = 0: the substitution, whose forms agree bit for bit) the covariance of the first 129
    points is the leading block of that of all 257, bit for bit: an entry does not depend on the grid it is computed in."""
    c = case(kind, N, D, max(FULL_COV_MS))
    g = fitted(ctx, c)
    Co, _, C64 = c.both("cov", lambda p: p.covariance(c.Xcs))
    (mu_o, _), (dev_mu, _), _ = c.both("predict", lambda p: p.predict(c.Xcs))
    worst = []
    try:
        for y_mean, y_std in TRANSFORMS:
            g.set_output_transform(y_mean, y_std)
            s2 = y_std * y_std
            for m in FULL_COV_MS:
                label = "V1 %s N=%d m=%d y_std=%g" % (kind, N, m, y_std)
                name = producer(ctx, g, c.Xc[:m])
                want = Co[:m, :m]
                dev = float(np.max(np.abs(C64[:m, :m] - want)))
                tol = entry_tol(c, dev, y_std, name)
                mean, C = g.predict_cov(c.Xc[:m])
                assert C.shape == (m, m) and np.all(np.isfinite(C)) and np.all(np.isfinite(mean)), label
                err = np.abs(C - want * L(s2)).astype(np.float64)
                worst.append(_report(label + " entries (%s)" % name, err, np.full(err.shape, tol)))
                assert float(err.max()) <= VAR_ATOL_REL_AMP * c.kscale * s2, label
                assert bits(C, C.T), label + ": not symmetric bit for bit"
                mu_p, var_p = g.predict(c.Xc[:m])
                err_d = np.abs(np.maximum(np.diag(C), EPS) - var_p)
                worst.append(_report(label + " diagonal vs predict", err_d, np.full(m, tol)))
                mo = (mu_o[:m] * L(y_std) + L(y_mean)).astype(np.float64)
                tol_mu = (MU_RTOL * np.abs(mu_o[:m]).astype(np.float64) +
                          MU_ATOL * max(1.0, float(np.abs(mu_o).max())) + HEADROOM * dev_mu) * y_std
                worst.append(_report(label + " mean", np.abs(mean - mo), tol_mu))
        # (still under the second transform: y_std^2 multiplies every entry of both)
        ctx.set_tuning("winv_max", 0)
        _, C257 = g.predict_cov(c.Xc[:257])
        _, C129 = g.predict_cov(c.Xc[:129])
        assert bits(C129, C257[:129, :129]), "V1 %s N=%d: the leading block depends on the grid" % (kind, N)
    finally:
        ctx.set_tuning("winv_max", None)
        g.set_output_transform(0.0, 1.0)
    return _finish(worst)


def check_refusals(ctx):
    """V1: m = 16385 is ROBO_BAD_SHAPE (before anything is allocated or launched); an unfitted handle answers the reference's
    "trained first" error from all three entry points"""
    import pytest
    c = case("matern52", 257, 3, max(FULL_COV_MS))
    g = fitted(ctx, c)
    with pytest.raises(_lib.RoboBadShape, match="16384"):
        g.predict_cov(np.zeros((16385, c.D)))
    mean, C = g.predict_cov(c.Xc[:3])                          # the handle is as good as before
    assert np.all(np.isfinite(C)) and np.all(np.isfinite(mean))
    raw = _lib.DeviceGP(ctx, c.kind, c.N, c.D)
    cand, rep = _lib.Candidates(ctx, c.Xc[:5]), _lib.Candidates(ctx, c.Xc[5:8])
    try:
        raw.set_data(c.X, c.y)
        for call in (lambda: raw.predict_cov(c.Xc[:5]), lambda: raw.predict_grad(c.Xc[:5]),
                     lambda: _lib.cross_cov(raw, cand, rep)):
            with pytest.raises(Exception, match="trained first"):
                call()
    finally:
        cand.close()
        rep.close()
        raw.close()


# ---- V2: consumers x producers --------------------------------------------------------------------------------------------------
# (label, tuning, kernel of predict_cov's stand-in, kernel of cross_cov's candidate handle, family).  cross_cov does not end
# in a synchronisation of its own that looks at the chain's time-out word, so it never takes the chained form
# (api_internal.h predict_core allow_chain): under trsm_chain = 1 its handles read the step kernel.
SUBSTITUTION = (
    ("launches", dict(winv_max=0, trsm_chain=0), STEP_SMALL, STEP_SMALL),
    ("chained", dict(winv_max=0, trsm_chain=1), CHAIN, STEP_SMALL),
    ("narrow0 deep0", dict(winv_max=0, trsm_chain=0, trsm_small_narrow=0, trsm_small_deep=0), STEP_SMALL, STEP_SMALL),
    ("narrow0 deep1", dict(winv_max=0, trsm_chain=0, trsm_small_narrow=0, trsm_small_deep=1), STEP_SMALL, STEP_SMALL),
    ("narrow1 deep0", dict(winv_max=0, trsm_chain=0, trsm_small_narrow=1, trsm_small_deep=0), STEP_SMALL, STEP_SMALL),
    ("narrow1 deep1", dict(winv_max=0, trsm_chain=0, trsm_small_narrow=1, trsm_small_deep=1), STEP_SMALL, STEP_SMALL),
    ("128-candidate step", dict(winv_max=0, trsm_small_max=0), STEP_GEN, STEP_GEN),
    ("pairs of block rows", dict(winv_max=0, trsm_small_max=0, trsm_pair=1), STEP_PAIR, STEP_PAIR),
    ("stepwise", dict(predict_stepwise=1), STEPWISE, STEPWISE),
)
INVERSE = (
    ("W chunked units", dict(winv_min_blocks=2, winv_rows=0), WINV_GEMM, WINV_GEMM),
    ("W whole rows", dict(winv_min_blocks=2, winv_rows=1), WINV_ROW, WINV_ROW),
)
PRODUCER_KEYS = ("winv_max", "trsm_chain", "trsm_small_narrow", "trsm_small_deep", "trsm_small_max", "trsm_pair",
                 "predict_stepwise", "winv_min_blocks", "winv_rows")
PRODUCER_SHAPE = dict(N=384, M=130, nbs=(5, 12))


def check_producers(ctx, kind, D):
    """V2.  N = 384 (three block rows and the skipped trailing block), m = 130 (a ragged second tile), reference sets of 5 and
    12 points; every producer of V forced through the tuning keys, the kernel that ran asserted (for cross_cov: on both
    handles; for predict_cov: by the stand-in of `producer`), and for each of them predict_cov and cross_cov against the
    oracle.  The substitution producers agree with each other bit for bit on both matrices.  For the Fabolas kernel the
    stepwise form is outside that claim: its right-hand side comes from cross_gram_kernel, which sums the one-dimensional
    factors' exponents before it takes ONE exponential (gram.hip pair_cov, matern52_1d_split) where the generated tiles
    multiply the factors (predict.hip gen_tile_accumulate): the same entries to rounding, not to the bit.
    The matrix-vector form of W (at most 8 candidates) is checked on the first 1, 5 and 8 candidates."""
    N, M, nbs = PRODUCER_SHAPE["N"], PRODUCER_SHAPE["M"], PRODUCER_SHAPE["nbs"]
    c = case(kind, N, D, M, nb=max(nbs))
    g = fitted(ctx, c)
    Co, dev_c, C64 = c.both("cov", lambda p: p.covariance(c.Xcs))
    So, _, S64 = c.both("cross", lambda p: p.covariance(c.Xcs, c.Zs))
    assert float(So.min()) < -1e-4, float(So.min())                            # the clip at eps is exercised
    cand = _lib.Candidates(ctx, c.Xc)
    reps = dict((nb, _lib.Candidates(ctx, c.Z[:nb])) for nb in nbs)
    worst, first = [], {}
    try:
        for family, table in (("substitution", SUBSTITUTION), ("inverse", INVERSE)):
            for label, tuning, name_cov, name_cc in table:
                for key in PRODUCER_KEYS:
                    ctx.set_tuning(key, tuning.get(key))
                tag = "V2 %s %s" % (kind, label)
                got = producer(ctx, g, c.Xc)
                assert got == name_cov, (tag, got, name_cov)
                _, C = g.predict_cov(c.Xc)
                err = np.abs(C - Co).astype(np.float64)
                worst.append(_report(tag + " predict_cov", err, np.full(err.shape, entry_tol(c, dev_c, 1.0, name_cov))))
                assert bits(C, C.T), tag
                out = {"cov": C}
                for nb in nbs:
                    S = _lib.cross_cov(g, cand, reps[nb])
                    assert cand.solve_kernel() == name_cc and reps[nb].solve_kernel() == name_cc, \
                        (tag, nb, cand.solve_kernel(), reps[nb].solve_kernel())
                    want = np.maximum(So[:, :nb], L(EPS))
                    dev = float(np.max(np.abs(S64[:, :nb] - So[:, :nb])))
                    err = np.abs(S - want).astype(np.float64)
                    worst.append(_report(tag + " cross_cov nb=%d" % nb, err,
                                         np.full(err.shape, entry_tol(c, dev, 1.0, name_cc))))
                    assert float(err.max()) <= CROSS_CONTRACT_REL_AMP * c.kscale, (tag, nb)
                    out["cross%d" % nb] = S
                if family == "substitution" and not (kind == "fabolas" and name_cov == STEPWISE):
                    for key, val in out.items():
                        if key in first:
                            assert bits(val, first[key]), "%s: %s differs from the first substitution producer" % (tag, key)
                        else:
                            first[key] = val
        # the matrix-vector form: at most 8 candidates, the automatic choice of the product's form
        for key in PRODUCER_KEYS:
            ctx.set_tuning(key, None)
        ctx.set_tuning("winv_min_blocks", 2)
        for m in (1, 5, 8):
            tag = "V2 %s W matrix-vector m=%d" % (kind, m)
            got = producer(ctx, g, c.Xc[:m])
            assert got == WINV_GEMV, (tag, got)
            _, C = g.predict_cov(c.Xc[:m])
            dev = float(np.max(np.abs(C64[:m, :m] - Co[:m, :m])))
            err = np.abs(C - Co[:m, :m]).astype(np.float64)
            worst.append(_report(tag + " predict_cov", err, np.full(err.shape, entry_tol(c, dev, 1.0, WINV_GEMV))))
            assert bits(C, C.T), tag
            few = _lib.Candidates(ctx, c.Xc[:m])
            try:
                S = _lib.cross_cov(g, few, reps[5])
                assert few.solve_kernel() == WINV_GEMV and reps[5].solve_kernel() == WINV_GEMV, \
                    (tag, few.solve_kernel(), reps[5].solve_kernel())
            finally:
                few.close()
            dev = float(np.max(np.abs(S64[:m, :5] - So[:m, :5])))
            err = np.abs(S - np.maximum(So[:m, :5], L(EPS))).astype(np.float64)
            worst.append(_report(tag + " cross_cov nb=5", err, np.full(err.shape, entry_tol(c, dev, 1.0, WINV_GEMV))))
    finally:
        for key in PRODUCER_KEYS:
            ctx.set_tuning(key, None)
        cand.close()
        for rep in reps.values():
            rep.close()
    return _finish(worst)


# ---- V3: cross-covariance shapes, chunked workspaces, information gain --------------------------------------------------------------
CROSS_CASES = (("rbf", 128, 4, 129, 2), ("matern52", 130, 3, 300, 64), ("fabolas", 256, 4, 400, 37))


def _chunked(ctx, N, blocks=1):
    ctx.set_tuning("ws_bytes", blocks * 128 * n_pad_of(N) * 8)


def check_cross_cov(ctx, kind, N, D, M, nb):
    """V3.  (N, M, nb) = (128, 129, 2), (130, 300, 64), (256, 400, 37): the cross-covariance against the oracle with negative
    entries present (the library clips at eps like the reference's predict_variance: clipped entries compare against
    max(oracle y_std^2, eps)), under both output transforms; and the same call with a workspace of ONE 128-candidate block
    (ws_bytes = 128 n_pad 8: two to four passes, V indexed chunk-locally while the candidates and S are indexed globally)
    gives the same bits."""
    c = case(kind, N, D, M, nb=nb)
    g = fitted(ctx, c)
    So, dev, _ = c.both("cross", lambda p: p.covariance(c.Xcs, c.Zs))
    assert float(So.min()) < -1e-4, float(So.min())
    assert float(So[-1].max()) > 1e-4, float(So[-1].max())                     # the last row is not all clipped (Case)
    worst = []
    cand, rep = _lib.Candidates(ctx, c.Xc), _lib.Candidates(ctx, c.Z)
    try:
        for y_mean, y_std in TRANSFORMS:
            label = "V3 %s N=%d M=%d nb=%d y_std=%g" % (kind, N, M, nb, y_std)
            g.set_output_transform(y_mean, y_std)
            S = _lib.cross_cov(g, cand, rep)
            assert cand.chunk() == cand_pad(M), (label, cand.chunk())
            want = np.maximum(So * L(y_std * y_std), L(EPS))
            assert int(np.sum(want == L(EPS))) > 0, label
            err = np.abs(S - want).astype(np.float64)
            worst.append(_report(label, err, np.full(err.shape, entry_tol(c, dev, y_std, cand.solve_kernel()))))
            assert float(err.max()) <= CROSS_CONTRACT_REL_AMP * c.kscale, label
            _chunked(ctx, N)
            c2 = _lib.Candidates(ctx, c.Xc)
            try:
                S2 = _lib.cross_cov(g, c2, rep)
                assert c2.chunk() == 128 and cand_pad(M) // 128 >= 2, (label, c2.chunk())
            finally:
                c2.close()
                ctx.set_tuning("ws_bytes", None)
            assert bits(S2, S), label + ": the chunked workspace changes the bits"
    finally:
        ctx.set_tuning("ws_bytes", None)
        g.set_output_transform(0.0, 1.0)
        cand.close()
        rep.close()
    return _finish(worst)


def cand_pad(M):
    return (M + 127) // 128 * 128


def ig_state(c, rep_rows, n_outcomes=40, seed=5):
    """the EP state of entropy search at the case's first reference points, set up as tests/test_infogain.py::_setup does, from
    the ORACLE's belief there -> (EPState, dict of its tensors)"""
    nb = len(rep_rows)
    p = c.posterior(L)
    mu_b = p.predict(c.Zs[rep_rows])[0].astype(np.float64)
    var_b = p.covariance(c.Zs[rep_rows]).astype(np.float64)
    logP, dMu, dSig, dMM = epmgp.joint_min(mu_b, var_b, with_derivatives=True)
    lmb = np.random.RandomState(seed).randn(nb)
    W = IG.outcome_quantiles(n_outcomes)
    d = dict(logP=logP, dMu=dMu, dSig=dSig, dMM=dMM, lmb=lmb, W=W, sn2=c.noise)
    return _lib.EPState(logP, lmb, W, dMu, dSig, dMM), d


def ig_reference(c, d, rows, rep_rows, y_std=1.0):
    """the NumPy restatement of the reference's dH (oracle/ig_oracle.py) fed with the ORACLE's (v, s) at the given rows"""
    p = c.posterior(L)
    s2 = L(y_std * y_std)
    var_o = np.maximum(p.predict(c.Xcs[rows])[1] * s2, L(EPS)).astype(np.float64)
    S_o = np.maximum(p.covariance(c.Xcs[rows], c.Zs[rep_rows]) * s2, L(EPS)).astype(np.float64)
    return np.array([IG.dh_fun(var_o[i], S_o[i][:, None], d["sn2"], d["logP"], d["lmb"], d["dMu"], d["dSig"], d["dMM"], d["W"])
                     for i in range(len(rows))])


def check_ig_chunked(ctx, kind="matern52", N=130, D=3, M=300, nb=64):
    """V3: information gain (Nb = 12 of the case's reference points, Np = 40) on one of the shapes.  The gains against the
    restatement fed with the oracle's (v, s) at the bound of tests/test_infogain.py; robo_ig_eval_cand with a workspace of one
    128-candidate block equals the single pass bit for bit: values, max and argmax.  The interpreter reports one CU, so there
    the single pass (3 tiles >= 2 x 1) takes the 128-row tile of cross_cov_kernel and gemm_nt_kernel and the chunked passes
    the 32-row tile: the promised "same k-order per entry, same bits"."""
    c = case(kind, N, D, M, nb=nb)
    g = fitted(ctx, c)
    rep_rows = np.arange(12)
    ep, d = c.memo("ig", lambda: ig_state(c, rep_rows))
    ref = c.memo("ig_ref", lambda: ig_reference(c, d, np.arange(M), rep_rows))
    cand, rep = _lib.Candidates(ctx, c.Xc), _lib.Candidates(ctx, c.Z[rep_rows])
    try:
        vals, mx, am = _lib.ig_eval(g, cand, rep, ep, d["sn2"])
        assert cand.chunk() == cand_pad(M)
        err = np.abs(vals - ref)
        r = _report("V3 information gain %s N=%d M=%d" % (kind, N, M), err, IG_RTOL * np.abs(ref) + IG_RTOL * np.abs(ref).max())
        assert r[0] <= 1.0, r[1]
        assert am == int(np.argmax(vals)) and mx == vals[am]
        _chunked(ctx, N)
        c2 = _lib.Candidates(ctx, c.Xc)
        try:
            vals2, mx2, am2 = _lib.ig_eval(g, c2, rep, ep, d["sn2"])
            assert c2.chunk() == 128
        finally:
            c2.close()
        assert bits(vals2, vals) and bits([mx2], [mx]) and am2 == am
    finally:
        ctx.set_tuning("ws_bytes", None)
        cand.close()
        rep.close()
    return r[0]


# ---- V4: input gradients --------------------------------------------------------------------------------------------------------
GRAD_CASES = (("matern52", 256, 3, 70), ("rbf", 128, 4, 40), ("fabolas", 130, 4, 40), ("matern52", 385, 3, 33))


def check_gradients(ctx, kind, N, D, M):
    """V4.  robo_gp_predict_grad (the C ABI form) against the oracle's analytic gradients (themselves pinned to central
    differences in long double, tests/test_v_consumers.py): N = 256 and 128 (N % 128 == 0: the trailing block is skipped and the
    dot products run over exactly n columns), 130 (ragged second block row), 385 (four block rows); unequal metrics per
    dimension; both output transforms.  Mean and variance equal `predict`'s at the bound parity_checks.check_predictive_gradients
    holds them to.  With a workspace of one 128-row block (ws_bytes = 128 n_pad 8) a pass holds 128 // (D + 1) candidates with
    tail pseudo-rows zeroed up to 128, so the call takes ceil(M / (128 // (D + 1))) >= 2 passes (the count follows from the
    rule's inputs; the ABI does not report it) and returns the same four arrays bit for bit."""
    c = case(kind, N, D, M)
    g = fitted(ctx, c)
    (dm_o, dv_o), (dev_m, dev_v), _ = c.both("grad", lambda p: p.gradients(c.Xcs, c.ism))
    tol_m = ENTRY_REL_AMP * float(np.abs(dm_o).max()) + HEADROOM * dev_m
    tol_v = ENTRY_REL_AMP * float(np.abs(dv_o).max()) + HEADROOM * dev_v
    worst = []
    try:
        for y_mean, y_std in TRANSFORMS:
            label = "V4 %s N=%d D=%d M=%d y_std=%g" % (kind, N, D, M, y_std)
            g.set_output_transform(y_mean, y_std)
            s2 = y_std * y_std
            one = g.predict_grad(c.Xc)
            mean, var, dm, dv = one
            assert all(np.all(np.isfinite(a)) for a in one), label
            err = np.abs(dm - dm_o * L(y_std)).astype(np.float64)
            worst.append(_report(label + " d mean / d x", err, np.full(err.shape, tol_m * y_std)))
            err = np.abs(dv - dv_o * L(s2)).astype(np.float64)
            worst.append(_report(label + " d var / d x", err, np.full(err.shape, tol_v * s2)))
            mu_p, var_p = g.predict(c.Xc)
            np.testing.assert_allclose(mean, mu_p, rtol=1e-11, atol=1e-12 * y_std)
            np.testing.assert_allclose(var, var_p, rtol=0, atol=1e-11 * c.kscale * s2)
            per = 128 // (D + 1)
            n_pass = -(-M // per)
            assert n_pass >= 2, n_pass
            print("%s: %d passes of %d candidates under a one-block workspace" % (label, n_pass, per))
            _chunked(ctx, N)
            try:
                many = g.predict_grad(c.Xc)
            finally:
                ctx.set_tuning("ws_bytes", None)
            for a, b, what in zip(one, many, ("mean", "variance", "d mean / d x", "d var / d x")):
                assert bits(a, b), "%s: %s differs between one pass and %d" % (label, what, n_pass)
    finally:
        ctx.set_tuning("ws_bytes", None)
        g.set_output_transform(0.0, 1.0)
    return _finish(worst)


# ---- V5: the 128-row tile ---------------------------------------------------------------------------------------------------------
_CU_COUNT = []


def device_cu_count():
    """torch.cuda.get_device_properties(0).multi_processor_count: hipDeviceProp_t::multiProcessorCount, the number api_ctx.hip
    reads into num_cu.  Asked in a fresh child process, once per test process: the torch wheel carries its own copy of the
    HIP runtime, and a second runtime finds no device in a process in which librobo_hip.so has already brought up its own
    ("No HIP GPUs are available")."""
    if not _CU_COUNT:
        import subprocess
        import sys
        code = "import torch; print(int(torch.cuda.get_device_properties(0).multi_processor_count))"
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        n = int(r.stdout.strip().splitlines()[-1])
        assert 1 <= n <= 4096, n
        _CU_COUNT.append(n)
    return _CU_COUNT[0]


def check_wide_tile(ctx, num_cu):
    """V5.  launch_cross_cov takes cross_cov_kernel<4, *> and launch_ig_dh gemm_nt_kernel<4> when a workspace pass holds at least
    2 num_cu tiles of 128 candidates (infogain.hip); num_cu is the device's multiprocessor count, the number api_ctx.hip reads.
    N = 256, D = 4, M = 256 num_cu + 5 (2 num_cu + 1 tiles, the last one ragged), nb = 12: the rule's own inputs are asserted
    from the handle's chunk.  cross_cov and ig_eval (Np = 40) at every 97th row and the last 6 against the oracle; then with
    ws_bytes = 128 num_cu n_pad 8 a pass holds num_cu tiles, the 32-row tile runs, and S, the gains, max and argmax are the
    same bits."""
    N, D, nb = 256, 4, 12
    M = 256 * num_cu + 5
    c = case("matern52", N, D, M, nb=nb, seed=num_cu)
    g = fitted(ctx, c)
    rows = np.unique(np.concatenate((np.arange(0, M, 97), np.arange(M - 6, M))))
    rep_rows = np.arange(nb)
    So, dev, _ = c.both("cross rows", lambda p: p.covariance(c.Xcs[rows], c.Zs))
    assert float(So.min()) < -1e-4 and float(So[-1].max()) > 1e-4, (float(So.min()), float(So[-1].max()))
    ep, d = c.memo("ig", lambda: ig_state(c, rep_rows))
    ref = c.memo("ig_ref", lambda: ig_reference(c, d, rows, rep_rows))
    worst = []
    cand, rep = _lib.Candidates(ctx, c.Xc), _lib.Candidates(ctx, c.Z)
    try:
        S = _lib.cross_cov(g, cand, rep)
        assert cand.chunk() // 128 >= 2 * num_cu, (cand.chunk(), num_cu)               # the 128-row tile's rule
        vals, mx, am = _lib.ig_eval(g, cand, rep, ep, d["sn2"])
        assert cand.chunk() // 128 >= 2 * num_cu, (cand.chunk(), num_cu)
        err = np.abs(S[rows] - np.maximum(So, L(EPS))).astype(np.float64)
        worst.append(_report("V5 cross_cov, 128-row tile (%d CUs, M=%d)" % (num_cu, M), err,
                             np.full(err.shape, entry_tol(c, dev, 1.0, cand.solve_kernel()))))
        assert float(err.max()) <= CROSS_CONTRACT_REL_AMP * c.kscale
        worst.append(_report("V5 information gain, 128-row tile", np.abs(vals[rows] - ref),
                             IG_RTOL * np.abs(ref) + IG_RTOL * np.abs(ref).max()))
        assert am == int(np.argmax(vals)) and mx == vals[am]
        ctx.set_tuning("ws_bytes", 128 * num_cu * n_pad_of(N) * 8)
        c2 = _lib.Candidates(ctx, c.Xc)
        try:
            S2 = _lib.cross_cov(g, c2, rep)
            assert c2.chunk() == 128 * num_cu and c2.chunk() // 128 < 2 * num_cu, (c2.chunk(), num_cu)   # the 32-row tile's
            vals2, mx2, am2 = _lib.ig_eval(g, c2, rep, ep, d["sn2"])
            assert c2.chunk() == 128 * num_cu, (c2.chunk(), num_cu)
        finally:
            c2.close()
        assert bits(S2, S), "V5: the cross-covariance differs between the 128-row and the 32-row tile"
        assert bits(vals2, vals) and bits([mx2], [mx]) and am2 == am, "V5: the gains differ between the two tiles"
    finally:
        ctx.set_tuning("ws_bytes", None)
        cand.close()
        rep.close()
    return _finish(worst)
