"""Plain oracle of the Bayesian linear regression (robo_amd/csrc/blr.hip): the device's arguments in, np.longdouble
throughout, no eigendecomposition and no sufficient statistics.  It forms Phi, factors A = beta Phi^T Phi + alpha I by Cholesky,
solves for m, forms y - Phi m explicitly and evaluates both forms of the marginal likelihood.
"""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def features(kind, X, omega=None, phase=None, scale=0.0):
    """-> Phi (n, F) in longdouble [, |x . omega| (n, F) for the random Fourier features' bound]"""
    X = np.asarray(X, dtype=LD)
    one = np.ones((X.shape[0], 1), dtype=LD)
    if kind == "given":
        return X
    if kind == "linear":
        return np.concatenate((X, one), axis=1)
    if kind == "quadratic":
        return np.concatenate((X * X, X, one), axis=1)
    arg = X @ np.asarray(omega, dtype=LD)
    return LD(scale) * np.cos(arg + np.asarray(phase, dtype=LD))


def rff_argument(X, omega):
    """sum_d |x_d omega_df|: what the rounding of the cosine's argument scales with"""
    return np.abs(np.asarray(X, dtype=LD)) @ np.abs(np.asarray(omega, dtype=LD))


def cholesky(A):
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_lower(L, B, trans=False):
    B = np.array(B, dtype=LD)
    n = L.shape[0]
    for i in (range(n - 1, -1, -1) if trans else range(n)):
        if trans:
            B[i] = (B[i] - L[i + 1:, i] @ B[i + 1:]) / L[i, i]
        else:
            B[i] = (B[i] - L[i, :i] @ B[:i]) / L[i, i]
    return B


class Posterior(object):
    """the weight-space posterior of one (alpha, beta)"""

    def __init__(self, Phi, y, alpha, beta):
        self.Phi, self.y, self.alpha, self.beta = np.asarray(Phi, dtype=LD), np.asarray(y, dtype=LD), LD(alpha), LD(beta)
        F = self.Phi.shape[1]
        self.L = cholesky(self.beta * (self.Phi.T @ self.Phi) + self.alpha * np.eye(F, dtype=LD))
        self.m = self.beta * solve_lower(self.L, solve_lower(self.L, self.Phi.T @ self.y), trans=True)

    def loglik(self, form):
        n, F = self.Phi.shape
        r = self.y - self.Phi @ self.m
        res = np.sqrt(r @ r) if form == 0 else r @ r
        return (F / LD(2) * np.log(self.alpha) + n / LD(2) * np.log(self.beta) - n / LD(2) * np.log(2 * LD(np.pi))
                - self.beta / 2 * res - self.alpha / 2 * (self.m @ self.m) - np.sum(np.log(np.diag(self.L))))

    def predict(self, phi):
        """-> mean, var (m,) at feature rows phi"""
        phi = np.asarray(phi, dtype=LD)
        V = solve_lower(self.L, phi.T)
        return phi @ self.m, 1 / self.beta + np.sum(V * V, axis=0)


def mixture(means, variances):
    """the reference's predict (:244-252) over per-sample moments (S, m)"""
    return np.mean(means, axis=0), np.maximum(np.mean(variances, axis=0), LD(EPS))
