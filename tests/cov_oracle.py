"""Extended-precision oracle of the covariance functions for tests/cov_checks.py.

Scalars in mpmath (50 digits), matrices / Cholesky / substitution in np.longdouble (x87 80-bit: 64-bit significand).  The
inputs are scaled in fp64 exactly as the device scales them -- x * ism_d with ism_d = exp(-0.5 ln m_d), one rounding --
so that oracle and device differ only in what follows the scaling (robo_amd/csrc/gram.hip scale_inputs_kernel)."""
import mpmath as mp
import numpy as np

L = np.longdouble
JITTER = 1.25e-12           # robo_amd/csrc/common.h
mp.mp.dps = 50


def inv_sqrt_metric(ln_m):
    return np.exp(-0.5 * np.asarray(ln_m, dtype=np.float64))


def scale(X, ln_m, n_scaled=None):
    """the device's scaled inputs (fp64); n_scaled: only the first columns carry a metric (Fabolas: all but the last)"""
    X = np.asarray(X, dtype=np.float64)
    ism = np.ones(X.shape[1])
    ln_m = np.broadcast_to(np.asarray(ln_m, dtype=np.float64), (X.shape[1] if n_scaled is None else n_scaled,))
    ism[:ln_m.size] = inv_sqrt_metric(ln_m)
    return X * ism[None, :]


# ---- scalars (mpmath) ---------------------------------------------------------------------------------------------------
def k_scalar(kind, r2):
    """matern52 / rbf at the squared scaled distance r2 (an exact mpf), unit amplitude"""
    r2 = mp.mpf(r2)
    if kind == "matern52":
        s = mp.sqrt(5 * r2)
        return (1 + s + 5 * r2 / 3) * mp.exp(-s)
    if kind == "rbf":
        return mp.exp(-r2 / 2)
    raise ValueError(kind)


def k_argument(kind, r2):
    """|argument of the exponential| at r2: what an error of the argument is amplified by"""
    r2 = np.asarray(r2, dtype=np.float64)
    with np.errstate(over="ignore"):
        return np.sqrt(5.0 * r2) if kind in ("matern52", "fabolas") else 0.5 * r2


def scalar_column(kind, x):
    """k(x_i, 0) for scalars x (exact doubles) -> (float64 nearest values, mpf list); fabolas: the one-dimensional factor"""
    vals = [k_scalar("matern52" if kind == "fabolas" else kind, mp.mpf(float(v)) ** 2) for v in x]
    return np.array([float(v) for v in vals]), vals


# ---- matrices (long double) -----------------------------------------------------------------------------------------------
def _matern_unit(r2):
    T = r2.dtype.type
    s = np.sqrt(T(5) * r2)
    return (T(1) + s + T(5) * r2 / T(3)) * np.exp(-s)


def kernel(kind, amp, A, B=None, blr=(1.0, 1.0), dtype=L):
    """k(A, B) on ALREADY SCALED rows by direct differences in `dtype` (np.longdouble: the oracle; np.float64: the fp64
    direct-difference model whose own deviation from the oracle the tolerances of check_feeds are built on).
    fabolas: the last column is the unscaled fidelity coordinate; blr = (a, b)."""
    A = np.asarray(A).astype(dtype)
    B = A if B is None else np.asarray(B).astype(dtype)
    T = np.dtype(dtype).type
    if kind == "fabolas":
        prod = np.ones((A.shape[0], B.shape[0]), dtype=dtype)
        for d in range(A.shape[1] - 1):
            diff = A[:, d][:, None] - B[:, d][None, :]
            prod *= _matern_unit(diff * diff)
        uu = A[:, -1][:, None] * B[:, -1][None, :]
        return T(amp) * prod * (T(blr[0]) + T(blr[1]) * uu)
    r2 = np.zeros((A.shape[0], B.shape[0]), dtype=dtype)
    for d in range(A.shape[1]):
        diff = A[:, d][:, None] - B[:, d][None, :]
        r2 += diff * diff
    if kind == "matern52":
        return T(amp) * _matern_unit(r2)
    if kind == "rbf":
        return T(amp) * np.exp(T(-0.5) * r2)
    raise ValueError(kind)


def cholesky(K):
    """lower Cholesky factor in K's own precision (row-oriented, vectorised over the finished columns)"""
    K = np.array(K)
    n = K.shape[0]
    Lf = np.zeros_like(K)
    for j in range(n):
        d = K[j, j] - Lf[j, :j] @ Lf[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite at column %d" % j)
        Lf[j, j] = np.sqrt(d)
        if j + 1 < n:
            Lf[j + 1:, j] = (K[j + 1:, j] - Lf[j + 1:, :j] @ Lf[j, :j]) / Lf[j, j]
    return Lf


def solve_lower(Lf, B):
    """L^-1 B by forward substitution in L's precision"""
    B = np.array(B, dtype=Lf.dtype)
    X = np.zeros_like(B)
    for i in range(Lf.shape[0]):
        X[i] = (B[i] - Lf[i, :i] @ X[:i]) / Lf[i, i]
    return X


class Posterior(object):
    """fit + predict of one theta in one precision, from the scaled rows"""

    def __init__(self, kind, amp, noise, Xs, y, mean, blr=(1.0, 1.0), dtype=L):
        T = np.dtype(dtype).type
        self.kind, self.amp, self.blr, self.dtype, self.Xs, self.mean = kind, amp, blr, dtype, Xs, mean
        K = kernel(kind, amp, Xs, blr=blr, dtype=dtype)
        K[np.diag_indices_from(K)] += T(noise) + T(JITTER)
        self.K = K
        self.Lf = cholesky(K)
        self.z = solve_lower(self.Lf, (np.asarray(y, dtype=np.float64) - mean).astype(dtype))
        n = K.shape[0]
        self.loglik = -T(0.5) * (self.z @ self.z + T(2) * np.sum(np.log(np.diag(self.Lf))) + T(n) * np.log(T(2) * T(np.pi)))

    def predict(self, Xcs):
        """(mean, variance) at scaled candidate rows; the variance is NOT floored"""
        Ks = kernel(self.kind, self.amp, Xcs, self.Xs, blr=self.blr, dtype=self.dtype)
        V = solve_lower(self.Lf, Ks.T)
        mu = V.T @ self.z + np.dtype(self.dtype).type(self.mean)
        T = np.dtype(self.dtype).type
        if self.kind == "fabolas":
            u = np.asarray(Xcs)[:, -1].astype(self.dtype)
            self_k = T(self.amp) * (T(self.blr[0]) + T(self.blr[1]) * u * u)
        else:
            self_k = np.full(Ks.shape[0], T(self.amp))
        return mu, self_k - np.sum(V * V, axis=0)

    def covariance(self, Xa_s, Xb_s=None):
        """posterior covariance k(a, b) - v_a . v_b between scaled rows (Xb_s None: Xa_s with itself); signed, NOT floored"""
        Va = solve_lower(self.Lf, kernel(self.kind, self.amp, Xa_s, self.Xs, blr=self.blr, dtype=self.dtype).T)
        Vb = Va if Xb_s is None else \
            solve_lower(self.Lf, kernel(self.kind, self.amp, Xb_s, self.Xs, blr=self.blr, dtype=self.dtype).T)
        return kernel(self.kind, self.amp, Xa_s, Xb_s, blr=self.blr, dtype=self.dtype) - Va.T @ Vb

    def grad_loglik(self):
        """(g, S): the gradient of the log marginal likelihood in the log-space hyper-parameters
        [ln amp, ln m_d ..., (ln a, ln b,) NOISE], and the magnitude each sum is conditioned by, in the instance's precision:
            W = L^-1,  alpha = W^T z,  A = alpha alpha^T - W^T W,
            g_p = 1/2 sum_ij A_ij dK_ij / d theta_p,      S_p = 1/2 sum_ij |A_ij dK_ij / d theta_p|
        with dK / d theta_p by the formulas of oracle.gp_oracle.kernel_gradient, on the SCALED rows (d r2 / d ln m_d =
        -(xs_d - xs'_d)^2).  The last entry is 1/2 tr A: the derivative in sigma^2, not in ln sigma^2 (the reference's grad_nll,
        DESIGN.md "Mirrored quirks").  One dK / d theta_p exists at a time (D = 256 would otherwise hold 256 N x N matrices)."""
        T = np.dtype(self.dtype).type
        n = self.K.shape[0]
        W = solve_lower(self.Lf, np.eye(n, dtype=self.dtype))
        alpha = W.T @ self.z
        KI = np.zeros((n, n), dtype=self.dtype)
        for r0 in range(0, n, 64):                                          # W is lower triangular: rows r0.. reach columns < r0 + 64
            r1 = min(r0 + 64, n)
            KI[:r1, :r1] += W[r0:r1, :r1].T @ W[r0:r1, :r1]
        A = np.outer(alpha, alpha) - KI
        X = np.asarray(self.Xs).astype(self.dtype)
        Kc = kernel(self.kind, self.amp, X, blr=self.blr, dtype=self.dtype)  # without the noise on the diagonal
        g, S = [], []

        def add(dK):
            t = A * dK
            g.append(T(0.5) * np.sum(t))
            S.append(T(0.5) * np.sum(np.abs(t)))
        add(Kc)                                                             # d / d ln amp
        fab = self.kind == "fabolas"
        d_in = X.shape[1] - 1 if fab else X.shape[1]
        if fab:
            for d in range(d_in):
                diff = X[:, d][:, None] - X[:, d][None, :]
                s = diff * diff
                t = np.sqrt(T(5) * s)
                add(Kc * (T(5) / T(6)) * (T(1) + t) * s / (T(1) + t + T(5) * s / T(3)))
            uu = X[:, -1][:, None] * X[:, -1][None, :]
            B = T(self.blr[0]) + T(self.blr[1]) * uu
            add(Kc * T(self.blr[0]) / B)
            add(Kc * T(self.blr[1]) * uu / B)
        else:
            if self.kind == "matern52":
                r2 = np.zeros((n, n), dtype=self.dtype)
                for d in range(d_in):
                    diff = X[:, d][:, None] - X[:, d][None, :]
                    r2 += diff * diff
                t = np.sqrt(T(5) * r2)
                dk = -T(self.amp) * (T(5) / T(6)) * (T(1) + t) * np.exp(-t)   # amp f'(r2)
            elif self.kind == "rbf":
                dk = T(-0.5) * Kc
            else:
                raise ValueError(self.kind)
            for d in range(d_in):
                diff = X[:, d][:, None] - X[:, d][None, :]
                add(dk * (-(diff * diff)))
        add(np.eye(n, dtype=self.dtype))                                    # the mirrored quirk: d / d sigma^2
        return np.array(g, dtype=self.dtype), np.array(S, dtype=self.dtype)

    def gradients(self, Xcs, inv_sqrt_metric):
        """(d mean / d x, d variance / d x), each (M, D), at scaled candidate rows, in the UNSCALED input space:
        inv_sqrt_metric (D,) = d xs_d / d x_d (1 for the Fabolas fidelity column).  With v = L^-1 k_*, w_d = L^-1 d k_* / d xs_d:
            d mean / d xs_d = w_d . z,      d var / d xs_d = d k(x, x) / d xs_d - 2 v . w_d
        (robo_amd/csrc/predgrad.hip).  Stationary kernels k = amp f(r2): d k / d xs_d = amp f'(r2) 2 (xs_d - xs'_d), f' =
        -(5/6)(1 + t) e^-t (Matern 5/2, t = sqrt(5 r2)) or -f / 2 (RBF); k(x, x) is constant.  Fabolas k = amp prod_d m(df_d^2)
        (a + b u u'): the same with the one-dimensional factor, d k / d u = amp prod b u' and d k(x, x) / d u = 2 amp b u."""
        T = np.dtype(self.dtype).type
        A, B = np.asarray(Xcs).astype(self.dtype), np.asarray(self.Xs).astype(self.dtype)
        M, D = A.shape
        diff = A[:, None, :] - B[None, :, :]                                # (M, N, D)
        dK = np.empty((D,) + diff.shape[:2], dtype=self.dtype)
        dself = np.zeros((M, D), dtype=self.dtype)
        if self.kind == "fabolas":
            a, b = T(self.blr[0]), T(self.blr[1])
            s2 = diff[:, :, :-1] ** 2
            t = np.sqrt(T(5) * s2)
            fac = (T(1) + t + T(5) * s2 / T(3)) * np.exp(-t)               # the factors m(df_d^2)
            dfac = -(T(5) / T(6)) * (T(1) + t) * np.exp(-t) * T(2) * diff[:, :, :-1]
            uu = A[:, -1][:, None] * B[:, -1][None, :]
            for d in range(D - 1):
                others = np.prod(np.delete(fac, d, axis=2), axis=2)
                dK[d] = T(self.amp) * others * dfac[:, :, d] * (a + b * uu)
            dK[D - 1] = T(self.amp) * np.prod(fac, axis=2) * b * B[:, -1][None, :]
            dself[:, D - 1] = T(2) * T(self.amp) * b * A[:, -1]
        else:
            r2 = np.sum(diff * diff, axis=2)
            if self.kind == "matern52":
                t = np.sqrt(T(5) * r2)
                df = -(T(5) / T(6)) * (T(1) + t) * np.exp(-t)
            elif self.kind == "rbf":
                df = T(-0.5) * np.exp(T(-0.5) * r2)
            else:
                raise ValueError(self.kind)
            for d in range(D):
                dK[d] = T(self.amp) * df * T(2) * diff[:, :, d]
        V = solve_lower(self.Lf, kernel(self.kind, self.amp, Xcs, self.Xs, blr=self.blr, dtype=self.dtype).T)
        dm, dv = np.empty((M, D), dtype=self.dtype), np.empty((M, D), dtype=self.dtype)
        ism = np.asarray(inv_sqrt_metric, dtype=np.float64).astype(self.dtype)
        for d in range(D):
            Wd = solve_lower(self.Lf, dK[d].T)
            dm[:, d] = (Wd.T @ self.z) * ism[d]
            dv[:, d] = (dself[:, d] - T(2) * np.sum(V * Wd, axis=0)) * ism[d]
        return dm, dv
