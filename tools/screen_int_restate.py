"""CPU restatement of the integer first stage's rule at the benchmark's seeded inputs (no GPU, NumPy only).

For the headline (N = 4096, D = 16) and config 2 (N = 1024, D = 8), 65 536 candidates, EI at eta = min y: the grid step h, the
first stage's whole term in units of the prior standard deviation (screen.hip "The integer form"), how many candidates fall
outside the grid's range, and how many survive when that term is added to every mean (U_c at the prior variance, L_c at the
variance floor), next to today's fp64-MFMA first stage.  One JSON line per shape.
"""
import json
import math
import sys

import numpy as np
from scipy.special import ndtr

SINGLE_EPS, SAFETY, AMAX, GRID = 6.3e-7, 1.5, 8355711, 8355000.0     # screen.hip: SD_SINGLE_EPS, SCREEN_SINGLE_SAFETY, SD_INT_*


def matern52(A, B):
    r2 = np.maximum((A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * A @ B.T, 0.0)
    s = np.sqrt(5.0 * r2)
    return (1.0 + s + s * s / 3.0) * np.exp(-s)


def ei(m, v, eta):
    sd = np.sqrt(v)
    z = (eta - m) / sd
    return (eta - m) * ndtr(z) + sd * np.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)


def restate(N, D, M=65536):
    X = np.random.RandomState(0).rand(N, D)
    y = np.sinc(X * 10 - 5).sum(axis=1)
    y = (y - y.mean()) / y.std()
    Xc = np.random.RandomState(1).rand(M, D)
    ell = math.sqrt(0.25 * D)
    Xs, Xcs = X / ell, Xc / ell
    K = matern52(Xs, Xs) + (1e-3 + 1.25e-12) * np.eye(N)
    alpha = np.linalg.solve(K, y - y.mean())
    asum = float(np.abs(alpha).sum())
    ctr = 0.5 * (Xs.max(0) + Xs.min(0))
    H = float(np.abs(Xs - ctr).max())
    h = 2.0 * H / GRID
    out_of_range = int((np.abs(np.rint((Xcs - ctr) / h)) > AMAX).any(axis=1).sum())
    e_int = 0.63 * math.sqrt(D) * h + (5.0 / 6.0) * 2.0 ** 20 * h * h
    mu = np.concatenate([matern52(Xcs[a:a + 4096], Xs) @ alpha for a in range(0, M, 4096)]) + y.mean()
    eta = float(y.min())
    res = dict(N=N, D=D, M=M, sum_abs_alpha=asum, H=H, h=h, e_int=e_int, out_of_range=out_of_range)
    for name, eps in (("fp64_mfma", SINGLE_EPS), ("int8", SINGLE_EPS + e_int)):
        delta = SAFETY * eps * asum
        up, lo = ei(mu - delta, 1.0 + 1e-5, eta), ei(mu + delta, 2.220446049250313e-16, eta)
        res[name] = dict(term=delta, survivors=int((up >= lo.max()).sum()))
    return res


if __name__ == "__main__":
    for N, D in ((4096, 16), (1024, 8)) if len(sys.argv) < 3 else ((int(sys.argv[1]), int(sys.argv[2])),):
        print(json.dumps(restate(N, D)), flush=True)
