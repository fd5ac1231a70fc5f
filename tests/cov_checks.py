"""Every covariance path of the library against the extended-precision oracle (tests/cov_oracle.py), over the argument range
and at the hyper-parameters the priors really reach (ln metric in [-10, 2]: scaled coordinates up to x e^5).

The same functions run in two settings, as those of parity_checks.py do:
  * tests/test_covariance.py   (-m gpu): librobo_hip.so on an MI355X;
  * tests/test_emu_covariance.py  (CPU): the interpreted build of the same sources (its rsq is exact and its exp / sqrt are
    the host's: only the GPU run says anything about pos_sqrt and the hardware's expf).
The paths: the fp64 gram tile in its dot and direct-difference forms (robo_gp_get_gram), the fp32 and the Fabolas tile
(pair_cov), the cross-gram kernel and the scalar cov_rows (diagnostics entry points, include/robo_hip_diag.h), and what
the entries feed: fit, the batched fits, the gradient's likelihood, the chain kernels' log-probabilities, predict.

Tolerances are derived, not measured (each function's docstring); every check prints its worst ratio (error / tolerance)
before it asserts, NOTES.md "covariance checks" records the ones measured on the hardware."""
import numpy as np

import cov_oracle as CO
from _tol import LOGLIK_RTOL, MU_ATOL, MU_RTOL, VAR_ATOL_REL_AMP
from oracle import gp_oracle as O
from robo_amd import _lib

L = np.longdouble
EPS64, EPS32 = 2.0 ** -52, 2.0 ** -23
SUBNORMAL64 = 2.0 ** -1074
FLT_MIN = 2.0 ** -126


# ---- C1: the scalar function over its whole argument range ---------------------------------------------------------------
def sweep_points(kind, fp32):
    """scalars x >= 0 (column 0 of K against x_0 = 0 is k(x^2)): r2 = x^2 logarithmic over the type's range, dense where the
    exponential's argument crosses 700 .. 746 (fp64: subnormal and underflowing results; fp32: 85 .. 104), and exact 0.
    fp32: every x is an fp32 number (the tile converts the staged fp64 coordinate), up to the largest one: from x = 1.8e19 on
    x^2, 5 r2 and the Fabolas factor's s^2 are inf in fp32 and the entry must still be 0, not inf * 0."""
    lo, hi = (-44.0, 76.0) if fp32 else (-300.0, 300.0)
    r2 = 10.0 ** np.linspace(lo, hi, 121)
    a0, a1 = (85.0, 104.0) if fp32 else (700.0, 746.0)
    arg = np.linspace(a0, a1, 47)
    dense = arg * arg / 5.0 if kind in ("matern52", "fabolas") else 2.0 * arg
    mid = 10.0 ** np.linspace(-3.0, 3.0, 25)                    # the O(1) range, where the entries matter
    x = np.sqrt(np.concatenate([r2, dense, mid]))
    if fp32:
        x = np.concatenate([x, [float(np.finfo(np.float32).max)]]).astype(np.float32).astype(np.float64)
    return np.concatenate([[0.0, 0.0], np.sort(x)])


def scalar_tolerance(kind, x, want, eps, floor):
    """relative eps (8 + 2 |a|), a the exponential's argument (sqrt(5 r2), r2 / 2), plus the absolute floor: one ulp each for
    5 r2, the square root and the range reduction, about 3 for the Horner polynomial and 3 for the closing products; an
    error of 1.5 ulp in a shows up as 1.5 a ulp of the exponential.
    The floor (one fp64 subnormal ulp; FLT_MIN in fp32, where a flush of denormals is allowed) is that of the EXPONENTIAL,
    which every form rounds to the type's grid before it multiplies by the Matern polynomial 1 + s + s^2 / 3: in the entry
    the floor is that many times larger (1.9e5 at s = 745: at s = 742 exp(-s) = 5.7e-323 has three significant bits)."""
    a = CO.k_argument(kind, x * x)
    poly = 1.0 + a + a * a / 3.0 if kind in ("matern52", "fabolas") else 1.0
    return eps * (8.0 + 2.0 * a) * np.abs(want) + floor * poly


def _report(label, err, tol, x=None):
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    w = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    msg = "%s: worst error / tolerance %.3g at %s" % (label, float(ratio[w]), (w,))
    if x is not None:
        msg += " (x = %r, error %.3g)" % (float(x[w]), float(err[w]))
    print(msg)
    return float(ratio[w]), msg


def check_scalar_sweep(ctx, kind, fp32):
    """C1 for one (kind, precision): the gram tile (dot and direct form in fp64: the sweep is cut where the tile changes),
    the cross-gram kernel and cov_rows, each against mpmath at the exact x_i^2"""
    x = sweep_points(kind, fp32)
    want, _ = CO.scalar_column(kind, x)
    eps, floor = (EPS32, FLT_MIN) if fp32 else (EPS64, SUBNORMAL64)
    tol = scalar_tolerance(kind, x, want, eps, floor)
    fab = kind == "fabolas"
    D = 2 if fab else 1
    theta = np.zeros(O.n_kernel_params(kind, D) + 1)       # ln m = 0: ism = 1, scaled = raw; amp = 1; fabolas a = b = 1
    theta[-1] = np.log(1e-3)

    def rows(v):               # fabolas: the fidelity column constant 1 -> a + b u u' = 2
        v = np.asarray(v, dtype=np.float64)[:, None]
        return np.hstack([v, np.ones_like(v)]) if fab else v
    factor = 2.0 if fab else 1.0
    worst = []
    # gram: the points behind x_0 = 0 in two data sets -- x^2 <= 500 keeps the fp64 stationary kernels on the dot tile
    # (common.h gram_needs_direct at D = 1, ln m = 0), the rest takes the direct-difference tile
    got = np.empty_like(x)
    cut = int(np.searchsorted(x, np.sqrt(500.0)))
    assert 0 < cut < x.size and cut <= 199 and x.size - cut <= 199
    for c0, c1 in ((0, cut), (cut, x.size)):
        xs = x[c0:c1]
        Xg = rows(np.concatenate([[0.0], xs]))
        g = _lib.DeviceGP(ctx, kind, Xg.shape[0], D)
        g.set_precision(fp32)
        g.set_data(Xg, np.zeros(Xg.shape[0]))
        K = g.gram(theta)
        got[c0:c1] = K[1:, 0]
        if c0 == 0:
            # the other two paths, whole sweep at once: the cross-gram of the one training point 0, cov_rows on pairs
            g1 = _lib.DeviceGP(ctx, kind, 1, D)
            g1.set_precision(fp32)
            g1.set_data(rows([0.0]), np.zeros(1))
            cross = g1.cross_gram(theta, rows(x))[:, 0]
            g1.close()
        g.close()
    paths = [("gram", got / factor), ("cross-gram", cross / factor)]
    if not fp32:
        cr = ctx.cov_rows(kind, rows(x), rows(np.zeros_like(x)), blr_a=1.0, blr_b=1.0)
        paths.append(("cov_rows", cr / factor))
    for name, val in paths:
        assert np.all(np.isfinite(val)), (kind, fp32, name, x[~np.isfinite(val)][:4])
        worst.append(_report("C1 %s %s %s" % (kind, "fp32" if fp32 else "fp64", name), np.abs(val - want), tol, x))
    bad = [m for r, m in worst if not r <= 1.0]
    assert not bad, bad
    return max(r for r, _ in worst)


# ---- C2: distance geometry ---------------------------------------------------------------------------------------------
def geometry_inputs(N, D, ln_m, seed, offset=0.0):
    """[0, 1]^D rows; the second half near-duplicates of the first at SCALED distance 1e-4; the last three rows exact
    duplicates of rows 0 .. 2 (off the diagonal); optionally everything shifted by `offset`"""
    rs = np.random.RandomState(seed)
    h = N // 2
    X = rs.rand(N, D)
    ism = CO.inv_sqrt_metric(np.broadcast_to(ln_m, (D,)))
    u = rs.randn(N - h, D)
    u /= np.linalg.norm(u, axis=1)[:, None]
    X[h:] = X[:N - h] + 1e-4 * u / ism[None, :]
    X[N - 3:] = X[:3]
    return X + offset


def mixed_metrics(D, seed):
    return np.random.RandomState(seed).choice([-10.0, -4.0, 0.0, 2.0], size=D)


GEOMETRY_GRID = tuple((D, N) for D in (1, 15, 16, 17, 33) for N in (63, 64, 126, 130, 200))
GEOMETRY_LNM = (-10.0, -4.0, 0.0, 2.0, "mixed")


def geometry_cases():
    """(D, N, ln m, offset): the whole grid, and two cases offset by +1000 (D = 3: the raw-X example of INTEGRATION.md)"""
    out = [(D, N, lnm, 0.0) for D, N in GEOMETRY_GRID for lnm in GEOMETRY_LNM]
    out.append((15, 126, 0.0, 1000.0))
    out.append((3, 64, 0.0, 1000.0))
    return out


GRAM_DIRECT_BOUND = 1e-12       # robo_amd/csrc/common.h


def gram_needs_direct(X, ln_m):
    """Python mirror of common.h gram_needs_direct: (D + 3) eps 2 sum_d ism_d^2 max_i x_id^2 > GRAM_DIRECT_BOUND.  The cases of
    this file stay a factor two or more away from the bound on either side, so the mirror need not round as the library does."""
    X = np.asarray(X, dtype=np.float64)
    ism = CO.inv_sqrt_metric(np.broadcast_to(ln_m, (X.shape[1],)))
    return bool((X.shape[1] + 3) * 2.0 * EPS64 * np.sum(ism * ism * np.max(X * X, axis=0)) > GRAM_DIRECT_BOUND)


def check_geometry(ctx, cases):
    """C2.  Every direct-difference path within rtol 1e-13 + atol 1e-15 amp of the long-double oracle (fp32: both times
    2^29, against the oracle on the fp32-rounded scaled rows -- the conversion is the design, the arithmetic is checked).
    The fp64 gram of the stationary kernels is a direct-difference path wherever the library's criterion (metrics and data
    extents, gram_needs_direct) says so and is held to that tolerance there; where the criterion keeps the dot form it
    additionally gets amp c (D + 3) eps (|xi|^2 + |xj|^2), c = 5/6 (Matern) or 1/2 (RBF): max |dk / dr2| times the bound of
    the expansion's error.  In the offset cases a second handle that received its data through fit_batch must build the
    same K bit for bit (it carries its own copy of the data extents)."""
    worst = {}

    def track(name, ratio_msg, case):
        r, msg = ratio_msg
        if r > worst.get(name, (0.0, ""))[0]:
            worst[name] = (r, "%s %s" % (case, msg))
    amp = 1.7
    for case in cases:
        D, N, lnm, offset = case
        lnm_v = mixed_metrics(D, 100 + D + N) if isinstance(lnm, str) else np.full(D, lnm)
        X = geometry_inputs(N, D, lnm_v, 7 * D + N, offset)
        Xs = CO.scale(X, lnm_v)
        n2 = np.sum(Xs.astype(L) ** 2, axis=1)
        for kind, c in (("matern52", 5.0 / 6.0), ("rbf", 0.5)):
            theta = np.concatenate([[np.log(amp)], lnm_v, [np.log(1e-3)]])
            Ko = CO.kernel(kind, amp, Xs)
            g = _lib.DeviceGP(ctx, kind, N, D)
            g.set_data(X, np.zeros(N))
            K = g.gram(theta) - (1e-3 + CO.JITTER) * np.eye(N)
            assert np.all(np.isfinite(K)), case
            direct = gram_needs_direct(X, lnm_v)
            tol = 1e-13 * np.abs(Ko) + 1e-15 * amp
            if not direct:
                tol = tol + amp * c * (D + 3) * EPS64 * (n2[:, None] + n2[None, :])
            np.fill_diagonal(tol, 1e-13 * amp + 1e-15 * amp + 2 * EPS64)      # exact entry + the noise added and removed
            name = "%s gram (%s tile)" % (kind, "direct" if direct else "dot")
            track(name, _report("C2 %s %s" % (name, case,), np.abs(K - Ko).astype(np.float64), tol.astype(np.float64)), case)
            if offset != 0.0:
                assert direct, case
                g2 = _lib.DeviceGP(ctx, kind, N, D)
                _, st = _lib.fit_batch([g, g2], np.vstack([theta, theta]), 0.0)
                assert st[0] == _lib.OK and st[1] == _lib.OK, case
                K2 = g2.gram(theta) - (1e-3 + CO.JITTER) * np.eye(N)
                g2.close()
                np.testing.assert_array_equal(K2, K)
            if kind == "matern52":
                # cross-gram against the training rows themselves and 16 fresh points; cov_rows on N pairs (i, i + N/2)
                Xc = np.vstack([X, np.random.RandomState(N).rand(16, D) + offset])
                Kc = g.cross_gram(theta, Xc)
                Kco = CO.kernel(kind, amp, CO.scale(Xc, lnm_v), Xs)
                track("cross-gram", _report("C2 cross-gram %s" % (case,), np.abs(Kc - Kco).astype(np.float64),
                                            (1e-13 * np.abs(Kco) + 1e-15 * amp).astype(np.float64)), case)
                j = (np.arange(N) + N // 2) % N
                cr = ctx.cov_rows(kind, Xs, Xs[j], amp=amp)
                cro = Ko[np.arange(N), j]
                track("cov_rows", _report("C2 cov_rows %s" % (case,), np.abs(cr - cro).astype(np.float64),
                                          (1e-13 * np.abs(cro) + 1e-15 * amp).astype(np.float64)), case)
                # fp32 entries
                g.set_precision(True)
                K32 = g.gram(theta) - (1e-3 + CO.JITTER) * np.eye(N)
                K32o = CO.kernel(kind, amp, Xs.astype(np.float32))
                s = 2.0 ** 29
                t32 = (s * 1e-13 * np.abs(K32o) + s * 1e-15 * amp).astype(np.float64)
                np.fill_diagonal(t32, t32.diagonal() + 2 * EPS64)
                track("fp32 gram", _report("C2 fp32 gram %s" % (case,), np.abs(K32 - K32o).astype(np.float64), t32), case)
            g.close()
        # the Fabolas tile: the same inputs as the D input columns, one fidelity column u in [0, 1]
        Xf = np.hstack([X, np.random.RandomState(D).rand(N, 1)])
        a, b = 0.8, 1.3
        theta = np.concatenate([[np.log(amp)], lnm_v, [np.log(a), np.log(b)], [np.log(1e-3)]])
        Xfs = CO.scale(Xf, lnm_v, n_scaled=D)
        Kfo = CO.kernel("fabolas", amp, Xfs, blr=(a, b))
        g = _lib.DeviceGP(ctx, "fabolas", N, D + 1)
        g.set_data(Xf, np.zeros(N))
        Kf = g.gram(theta) - (1e-3 + CO.JITTER) * np.eye(N)
        g.close()
        assert np.all(np.isfinite(Kf)), case
        scale_f = amp * (a + b)
        tf = (1e-13 * np.abs(Kfo) + 1e-15 * scale_f).astype(np.float64)
        np.fill_diagonal(tf, tf.diagonal() + 2 * EPS64)
        track("fabolas gram", _report("C2 fabolas gram %s" % (case,), np.abs(Kf - Kfo).astype(np.float64), tf), case)
    for name, (r, msg) in sorted(worst.items()):
        print("C2 worst %s: %s" % (name, msg))
    bad = [msg for r, msg in worst.values() if not r <= 1.0]
    assert not bad, bad
    return {k: v[0] for k, v in worst.items()}


# ---- C3: what the entries feed -----------------------------------------------------------------------------------------
FEED_CASES = ((63, 16), (126, 15), (200, 17))         # one tile (NG = 1 chain kernel), three groups (NG = 3), two panels (launch path)
FEED_LNM = (-10.0, -4.0)
FEED_NOISE = (np.exp(-13.0), 1e-3)


def check_feeds(ctx, N, D, kind="matern52"):
    """C3 for one data set: the C2 inputs with near-duplicates, ln m in {-10, -4} x noise in {e^-13, 1e-3}.  fit, loglik_batch,
    fit_batch, grad_loglik's likelihood, the chain's lnprob for prescribed start positions and predict at 64
    points (32 of them training inputs) against the long-double oracle.  Tolerance: the constants of _tol.py plus 20 x the
    deviation of the fp64 direct-difference model (same algorithm in np.float64) from the long-double oracle on the same
    inputs -- 20 is the head-room check_ill_conditioned documents between the blocked factorisation and LAPACK.  The
    gradient against fourth-order central differences of the device's own likelihood as tightly as check_grad_loglik
    demands (rtol 1e-8, atol 1e-9 of the largest entry)."""
    amp = 1.3
    thetas, info = [], []
    for lnm in FEED_LNM:
        for noise in FEED_NOISE:
            thetas.append(np.concatenate([[np.log(amp)], np.full(D, lnm), [np.log(noise)]]))
            info.append((lnm, noise))
    thetas = np.array(thetas)
    failures = []
    for ti, (lnm, noise) in enumerate(info):
        theta = thetas[ti]
        X = geometry_inputs(N, D, lnm, 7 * D + N)
        rs = np.random.RandomState(N + D)
        y = np.sin(3.0 * X[:, 0]) + X.sum(axis=1) / D + 0.05 * rs.randn(N)
        mean = float(y.mean())
        Xc = np.vstack([X[:32], rs.rand(32, D)])
        Xs, Xcs = CO.scale(X, np.full(D, lnm)), CO.scale(Xc, np.full(D, lnm))
        noise_eff = float(np.exp(theta[-1]))
        ref = CO.Posterior(kind, amp, noise_eff, Xs, y, mean)
        m64 = CO.Posterior(kind, amp, noise_eff, Xs, y, mean, dtype=np.float64)
        mu_o, var_o = ref.predict(Xcs)
        mu_m, var_m = m64.predict(Xcs)
        var_o, var_m = np.maximum(var_o, O.EPS), np.maximum(var_m, O.EPS)
        dev_ll = abs(float(m64.loglik - ref.loglik))
        dev_mu = float(np.max(np.abs(mu_m - mu_o)))
        dev_var = float(np.max(np.abs(var_m - var_o)))
        ll_o = float(ref.loglik)
        tol_ll = LOGLIK_RTOL * abs(ll_o) + 20.0 * dev_ll
        print("C3 N=%d D=%d ln m=%g noise=%.3g: loglik %.6f; fp64 direct model deviates by %.3g (loglik, %.3g relative) "
              "%.3g (mean) %.3g (variance); loglik tolerance %.3g" % (N, D, lnm, noise, ll_o, dev_ll, dev_ll / abs(ll_o),
                                                                        dev_mu, dev_var, tol_ll))
        g = _lib.DeviceGP(ctx, kind, N, D)
        g.set_data(X, y)
        got = {"fit": g.fit(theta, mean)}
        mu, var = g.predict(Xc)
        llb, st = g.loglik_batch(np.vstack([theta, thetas[0]]), mean)       # a batch that also holds another theta
        assert st[0] == _lib.OK
        got["loglik_batch"] = llb[0]
        g2 = _lib.DeviceGP(ctx, kind, N, D)
        llf, stf = _lib.fit_batch([g, g2], np.vstack([theta, theta]), mean)
        assert stf[0] == _lib.OK and stf[1] == _lib.OK
        got["fit_batch"] = llf[1]
        mu2, var2 = g2.predict(Xc)
        g2.close()
        llg, grad = g.grad_loglik(theta, mean)
        got["grad_loglik"] = llg
        # the chain's start evaluation.  N <= 63: the one-launch chain kernel with NG = 1; <= 126: NG = 3; above: the launch
        # path (proposal kernel, gram kernel with both tiles, factorisation, tail) on the device-formed FitSample::direct
        e0 = np.empty((0, 2, 2))
        _, lnp, _, _, _ = g.mcmc_run(mean, None, thetas, None, 0, e0, e0.astype(np.int32), e0)
        got["mcmc lnprob"] = lnp[ti]                       # (the other three walkers see this data set at their own thetas)
        for name, val in got.items():
            err = abs(val - ll_o)
            print("   %-12s %.10f  error %.3g = %.3g of the tolerance" % (name, val, err, err / tol_ll))
            if not err <= tol_ll:
                failures.append("%s N=%d D=%d ln m=%g noise=%.3g: error %.3g (%.3g relative), tolerance %.3g" %
                                (name, N, D, lnm, noise, err, err / abs(ll_o), tol_ll))
        for name, (m_, v_) in (("predict", (mu, var)), ("predict after fit_batch", (mu2, var2))):
            tol_mu = MU_RTOL * np.abs(mu_o) + MU_ATOL * max(1.0, float(np.abs(mu_o).max())) + 20.0 * dev_mu
            tol_var = VAR_ATOL_REL_AMP * amp + 20.0 * dev_var
            e_mu, e_var = float(np.max(np.abs(m_ - mu_o) / tol_mu)), float(np.max(np.abs(v_ - var_o)) / tol_var)
            print("   %-12s mean %.3g, variance %.3g of the tolerance" % (name, e_mu, e_var))
            if not (e_mu <= 1.0 and e_var <= 1.0):
                failures.append("%s N=%d D=%d ln m=%g noise=%.3g: mean %.3g variance %.3g of the tolerance" %
                                (name, N, D, lnm, noise, e_mu, e_var))
        # the gradient against the device's own likelihood: fourth-order central differences; the last entry is d / d sigma^2
        # (include/robo_hip.h): chain rule on the log-noise step.  Step: the difference quotient carries the likelihood's own
        # absolute error dl over h (dl ~ 1e-7 at the noise floor, where |ll| = 2e4 and every derivative in ln sigma^2 is of
        # that size: the data term is ~ exp(-ln sigma^2)) and a truncation of h^4 |ll| / 30; they balance at
        # h = (30 dl / |ll|)^(1/5) = 0.01, where both are below 1e-9 of the derivative
        h = 1e-2
        P = theta.size
        steps = np.concatenate([theta + s * h * np.eye(P) for s in (-2.0, -1.0, 1.0, 2.0)])
        f, stc = g.loglik_batch(steps, mean)
        assert np.all(stc == _lib.OK)
        f = f.reshape(4, P).astype(L)
        fd = ((f[0] - f[3]) + L(8) * (f[2] - f[1])) / L(12 * h)
        fd[-1] /= L(np.exp(theta[-1]))
        fd = fd.astype(np.float64)
        scale_g = float(np.max(np.abs(fd)))
        e_g = float(np.max(np.abs(grad - fd) / (1e-8 * np.abs(fd) + 1e-9 * scale_g)))
        print("   gradient vs central differences: %.3g of the tolerance" % e_g)
        if not e_g <= 1.0:
            failures.append("gradient N=%d D=%d ln m=%g noise=%.3g: %.3g of the tolerance" % (N, D, lnm, noise, e_g))
        g.close()
    assert not failures, failures


# ---- C4: Fabolas products --------------------------------------------------------------------------------------------
FABOLAS_CASES = ((True, 4), (True, 9), (True, 12), (True, 20), (False, 17), (False, 70))


def check_fabolas_products(ctx, fp32, d_in, N=70):
    """C4: every input length scale at ln m = -10, raw distances 0.33 and 1 per dimension between the rows (true entries 0 or
    subnormal off the duplicate pairs): every entry finite and within the C2 tolerance of the oracle, and the fit succeeds"""
    amp, a, b = 1.0, 1.0, 1.0
    rs = np.random.RandomState(d_in)
    levels = np.array([0.0, 0.33, 1.0])
    X = levels[rs.randint(0, 3, size=(N, d_in))]
    X[0] = rs.randint(0, 2, size=d_in)                    # rows 1 and 2: exactly 0.33 and exactly 1 from row 0 in EVERY dimension
    X[1] = X[0] + 0.33 * (1.0 - 2.0 * X[0])
    X[2] = 1.0 - X[0]
    X[N - 2:] = X[:2]                                     # exact duplicates: entries a + b u u'
    Xf = np.hstack([X, rs.rand(N, 1)])
    lnm = np.full(d_in, -10.0)
    theta = np.concatenate([[np.log(amp)], lnm, [np.log(a), np.log(b)], [np.log(1e-3)]])
    Xs = CO.scale(Xf, lnm, n_scaled=d_in)
    Ko = CO.kernel("fabolas", amp, Xs.astype(np.float32) if fp32 else Xs, blr=(a, b))
    g = _lib.DeviceGP(ctx, "fabolas", N, d_in + 1)
    g.set_precision(fp32)
    y = np.sin(3.0 * Xf.sum(axis=1))
    g.set_data(Xf, y)
    K = g.gram(theta) - (1e-3 + CO.JITTER) * np.eye(N)
    n_bad = int(np.sum(~np.isfinite(K)))
    assert n_bad == 0, "fabolas %s D_in=%d: %d entries of K are not finite" % ("fp32" if fp32 else "fp64", d_in, n_bad)
    s = 2.0 ** 29 if fp32 else 1.0
    tol = (s * 1e-13 * np.abs(Ko) + s * 1e-15 * amp * (a + b)).astype(np.float64)
    np.fill_diagonal(tol, tol.diagonal() + 2 * EPS64)
    r, msg = _report("C4 fabolas %s D_in=%d" % ("fp32" if fp32 else "fp64", d_in), np.abs(K - Ko).astype(np.float64), tol)
    assert r <= 1.0, msg
    ll = g.fit(theta, float(y.mean()))                    # raises LinAlgError when K is not positive definite
    assert np.isfinite(ll)
    g.close()
    return r
