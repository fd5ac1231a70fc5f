"""NumPy oracle of the greedy batch selection with fantasised picks (robo_amd/csrc/batch.hip, include/robo_hip.h).

The independent statement is "append the fantasy observation and refit": oracle.gp_oracle's free functions gp_compute /
gp_predict_diag on the grown data set, with theta, the constant mean and the output transform FROZEN at the real data's
values (the mean is passed explicitly, never re-estimated from the fantasies).  The rank-one formulas the device uses are
restated next to it (RankOne) so that the two can be compared without a device.
"""
import numpy as np

from oracle import gp_oracle as O

EPS = O.EPS


class FrozenGP(object):
    """one fitted GP whose theta / mean / (y_mean, y_std) stay where the real data put them; y is in the LATENT scale"""

    def __init__(self, kind, theta, X, y, mean, y_mean=0.0, y_std=1.0):
        self.kind, self.theta = kind, np.asarray(theta, dtype=np.float64)
        self.X, self.y, self.mean = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), float(mean)
        self.y_mean, self.y_std = float(y_mean), float(y_std)
        self.d0 = float(np.exp(self.theta[-1]) + O.JITTER)       # what the fit adds to the diagonal

    def grown(self, hist):
        """hist: [(x_j (D,), y_f in the output scale)] -> (X', y' latent)"""
        if not hist:
            return self.X, self.y
        Xa = np.vstack([self.X] + [np.atleast_2d(x) for x, _ in hist])
        ya = np.concatenate([self.y, [(yf - self.y_mean) / self.y_std for _, yf in hist]])
        return Xa, ya

    def refit_latent(self, Xc, hist):
        Xa, ya = self.grown(hist)
        L = O.gp_compute(self.kind, self.theta, Xa)
        return O.gp_predict_diag(self.kind, self.theta, L, Xa, ya, self.mean, Xc)

    def transform(self, mu, var):
        return mu * self.y_std + self.y_mean, np.clip(var * self.y_std ** 2, EPS, np.inf)

    def refit(self, Xc, hist):
        """transformed, floored (mean, var) of the candidates after append-and-refit"""
        return self.transform(*self.refit_latent(Xc, hist))

    def refit_longdouble(self, Xc, hist):
        """the same in np.longdouble (kernel entries in fp64, factorisation and solves extended): small N only"""
        Xa, ya = self.grown(hist)
        ld = np.longdouble
        K = O.kernel_matrix(self.kind, self.theta[:-1], Xa).astype(ld)
        K[np.diag_indices_from(K)] += ld(np.exp(self.theta[-1])) + ld(O.JITTER)
        n = K.shape[0]
        L = np.zeros_like(K)
        for c in range(n):
            L[c, c] = np.sqrt(K[c, c] - L[c, :c] @ L[c, :c])
            if c + 1 < n:
                L[c + 1:, c] = (K[c + 1:, c] - L[c + 1:, :c] @ L[c, :c]) / L[c, c]
        B = np.column_stack([O.kernel_matrix(self.kind, self.theta[:-1], Xa, Xc).astype(ld), (ya - self.mean).astype(ld)])
        for r in range(n):
            B[r] = (B[r] - L[r, :r] @ B[:r]) / L[r, r]
        V, z = B[:, :-1], B[:, -1]
        mu = V.T @ z + ld(self.mean)
        var = O.kernel_diag(self.kind, self.theta[:-1], Xc).astype(ld) - np.sum(V * V, axis=0)
        return mu, var


class RankOne(object):
    """the device's rule restated: latent state of every candidate, conditioned pick by pick"""

    def __init__(self, gp, Xc):
        self.gp, self.Xc = gp, np.asarray(Xc, dtype=np.float64)
        self.L = O.gp_compute(gp.kind, gp.theta, gp.X)
        self.mu, self.var = O.gp_predict_diag(gp.kind, gp.theta, self.L, gp.X, gp.y, gp.mean, self.Xc)
        self.Ks = O.kernel_matrix(gp.kind, gp.theta[:-1], self.Xc, gp.X)          # (M, N)
        self.C = np.zeros((0, self.Xc.shape[0]))                                  # earlier c_j(x) / sqrt(d_j)

    def moments(self):
        return self.gp.transform(self.mu, self.var)

    def condition(self, j, yf):
        import scipy.linalg as sla
        gp = self.gp
        beta = sla.cho_solve((self.L, True), self.Ks[j], check_finite=False)
        c = O.kernel_matrix(gp.kind, gp.theta[:-1], self.Xc, self.Xc[j:j + 1])[:, 0] - self.Ks @ beta
        c = c - self.C.T @ self.C[:, j]               # the posterior covariance after the earlier picks
        d = self.var[j] + gp.d0
        innov = (yf - gp.y_mean) / gp.y_std - self.mu[j]
        self.mu = self.mu + c * innov / d
        self.var = self.var - c * c / d
        self.C = np.vstack([self.C, c / np.sqrt(d)])


def acquisition(kind, par, eta, mean, var):
    if kind == "ei":
        return O.ei(mean, var, eta, par)
    if kind == "log_ei":
        return O.log_ei_vec(mean, var, eta, par)
    if kind == "pi":
        return O.pi(mean, var, eta, par)
    return O.lcb(mean, var, par)


def marginal_values(kind, par, etas, means, vars_):
    """(S, M) moments -> the mean over the samples, accumulated in sample order"""
    acc = None
    for s in range(len(etas)):
        a = acquisition(kind, par, etas[s], means[s], vars_[s])
        acc = a if acc is None else acc + a
    return acc / float(len(etas))
