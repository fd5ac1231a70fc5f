"""The rule of robo_paths_create / robo_paths_eval_cand (include/robo_hip.h) in np.longdouble, on cov_oracle's kernel, Cholesky
and forward substitution plus a back substitution.  Fed the device's own doubles: scaled rows as cov_oracle.scale makes them
and the same omega, phase, w, eps.  The same routine with dtype=np.float64 is the plain-fp64 model whose deviation from the
long-double oracle the value bound of tests/test_paths.py is built on."""
import numpy as np

import cov_oracle as CO

LD = np.longdouble


def solve_upper(U, B):
    """U^-1 B by back substitution in U's precision"""
    B = np.array(B, dtype=U.dtype)
    X = np.zeros_like(B)
    for i in range(U.shape[0] - 1, -1, -1):
        X[i] = (B[i] - U[i, i + 1:] @ X[i + 1:]) / U[i, i]
    return X


def features(amp, A, omega, phase, dtype=LD):
    """phi(A) (rows x F) at ALREADY SCALED rows: sqrt(2 amp / F) cos(A omega^T + b)"""
    T = np.dtype(dtype).type
    A, omega, phase = (np.asarray(v).astype(dtype) for v in (A, omega, phase))
    F = omega.shape[0]
    return np.sqrt(T(2) * T(amp) / T(F)) * np.cos(A @ omega.T + phase[None, :])


class Paths(object):
    """alpha of every path once; values at any scaled candidate rows"""

    def __init__(self, kind, amp, noise, Xs, y, mean, omega, phase, w, eps, y_mean=0.0, y_std=1.0, dtype=LD):
        T = np.dtype(dtype).type
        self.kind, self.amp, self.dtype, self.mean = kind, amp, dtype, T(mean)
        self.Xs, self.omega, self.phase = Xs, omega, phase
        self.w = np.asarray(w).astype(dtype)                           # (S, F)
        self.y_mean, self.y_std = T(y_mean), T(y_std)
        K = CO.kernel(kind, amp, Xs, dtype=dtype)
        K[np.diag_indices_from(K)] += T(noise) + T(CO.JITTER)
        Lf = CO.cholesky(K)
        PhiX = features(amp, Xs, omega, phase, dtype)                  # (N, F)
        sd = np.sqrt(T(noise) + T(CO.JITTER))
        r = (np.asarray(y, dtype=np.float64).astype(dtype) - T(mean))[None, :] - self.w @ PhiX.T \
            - sd * np.asarray(eps).astype(dtype)                       # (S, N)
        self.alpha = solve_upper(Lf.T, CO.solve_lower(Lf, r.T)).T      # (S, N)

    def values(self, Xcs):
        """(S, m) at scaled candidate rows, output transform applied"""
        Ks = CO.kernel(self.kind, self.amp, Xcs, self.Xs, dtype=self.dtype)
        f = self.mean + self.w @ features(self.amp, Xcs, self.omega, self.phase, self.dtype).T + self.alpha @ Ks.T
        return f * self.y_std + self.y_mean


def np_argmax_neg(f):
    """per path np.argmax(-f): first index, NaN maximal"""
    return np.array([int(np.argmax(-np.asarray(row, dtype=np.float64))) for row in np.atleast_2d(f)], dtype=np.int64)
