"""NumPy restatement of the constrained value and its gradient as robo_cei_refine_cand forms them at a trial point
(include/robo_hip.h; robo_amd/csrc/cei_refine.hip), for tests/test_cei_refine.py.  Test infrastructure only.

A model is (OracleGP, y_mean, y_std): the fp64 oracle GP (oracle/gp_oracle.py, normalize_input=False, inputs in [0, 1]^D)
and the output transform the device GP carries.  Per model refine_oracle.moments gives m, v, dm, dv; then

    z_k = (t_k - m_k) / s_k,   L = sum_k log Phi(z_k),   dL = sum_k r(z_k) dz_k,   r = phi / Phi,
    dz_k = (-dm_k - z_k ds_k) / s_k,   ds = dv / (2 s)
    "log_ei":  f0 + L,  g0 + dL        "ei":  f0 exp(L),  exp(L) (g0 + f0 dL)        eta None:  L, dL  resp.  exp(L), exp(L) dL

with log Phi and r from cei_oracle.norm_cdf_pair in np.longdouble (continued fraction on the left: no underflow, no
cancellation) and the objective's f0, g0 from refine_oracle.acq_value_grad.  `ratio64` is the device's fp64 form of r
(plain quotient for z >= -1, reciprocal Mills ratio through erfcx below) for the comparison of the two.

THE VALUE'S BOUND.  The device's moments differ from the oracle's by what tests/_tol.py holds the posterior to:
|dm| <= MU_RTOL |m| + MU_ATOL y_std, |dv| <= VAR_ATOL_REL_AMP amp y_std^2.  log Phi answers them by its conditioning,
|dl_k| <= r_k (|dm_k| / s_k + |z_k| |dv_k| / (2 v_k)), summed over the constraints: moments_L.  The objective factor computed from
device moments is held to ACQ_RTOL relative (tests/test_refine.py).  On top comes cei_oracle's own bound of the fold on given
moments (rounding of the rule's operations).  Hence
    "log_ei":  ACQ_RTOL |f0| + moments_L + fold        "ei":  |value| (ACQ_RTOL + moments_L) + fold
    eta None:  moments_L + fold  resp.  |value| moments_L + fold
"""
import numpy as np
from scipy.special import erfcx

import cei_oracle as CO
import refine_oracle as RO
from _tol import ACQ_RTOL, MU_ATOL, MU_RTOL, VAR_ATOL_REL_AMP
from oracle import gp_oracle as O

LD = CO.LD
EPS_FLOOR = np.finfo(np.float64).eps


def model_moments(model, X):
    """(m, v, dm, dv, floored) of one (OracleGP, y_mean, y_std) with the transform applied and the variance floored at
    DBL_EPSILON as the device floors it (the gradient is the unclipped function's)"""
    ogp, y_mean, y_std = model
    m, v, dm, dv = RO.moments(ogp, X)
    m, v, dm, dv = m * y_std + y_mean, v * y_std ** 2, dm * y_std, dv * y_std ** 2
    floored = ~(v >= EPS_FLOOR)
    return m, np.where(floored, EPS_FLOOR, v), dm, dv, floored


def ratio64(z):
    """phi / Phi the way the device evaluates it in fp64"""
    z = np.atleast_1d(np.asarray(z, dtype=np.float64))
    out = np.empty_like(z)
    hi = z >= -1.0
    out[hi] = O.norm_pdf(z[hi]) / O.norm_cdf(z[hi])
    out[~hi] = 1.0 / (np.sqrt(np.pi / 2.0) * erfcx(-z[~hi] / np.sqrt(2.0)))
    return out


def evaluate(models, thresholds, kind, par, eta, X):
    """models[0]: the objective, models[1:]: the constraints -> dict(value, grad (M, D), bound, z (C, M), L, dL, floored (M,)
    over the models the device solves); value / bound / L in np.longdouble, the gradient in fp64"""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    M, D = X.shape
    thresholds = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    Cn = len(thresholds)
    assert len(models) == Cn + 1
    floored = np.zeros(M, dtype=bool)
    means, vars_, zs = np.zeros((Cn, M)), np.ones((Cn, M)), np.zeros((Cn, M))
    dL = np.zeros((M, D), dtype=LD)
    moments_L = np.zeros(M, dtype=LD)
    for k in range(Cn):
        m, v, dm, dv, fl = model_moments(models[1 + k], X)
        floored |= fl
        means[k], vars_[k] = m, v
        s = np.sqrt(v)
        z = (thresholds[k] - m) / s
        zs[k] = z
        _, _, mills = CO.norm_cdf_pair(z)
        ds = dv / (2.0 * s)[:, None]
        dz = (-dm - z[:, None] * ds) / s[:, None]
        dL = dL + mills[:, None] * dz.astype(LD)
        ogp, _, y_std = models[1 + k]
        tol_m = MU_RTOL * np.abs(m) + MU_ATOL * abs(y_std)
        tol_v = VAR_ATOL_REL_AMP * np.exp(ogp.theta[0]) * y_std ** 2
        moments_L = moments_L + mills * (tol_m / s + np.abs(z) * tol_v / (2.0 * v))
    if eta is not None or Cn == 0:
        m0, v0, dm0, dv0, fl0 = model_moments(models[0], X)
        floored |= fl0
    else:
        m0, v0 = np.zeros(M), np.ones(M)          # (not read: the device leaves the objective's GP out of the iterations)
    fold = CO.cei_batch(m0, v0, means, vars_, thresholds, kind, par, eta)
    L = fold["L"]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        P = np.exp(L)
        if eta is not None:
            f0, g0 = RO.acq_value_grad(kind, par, eta, m0, v0, dm0, dv0)
            f0 = f0.astype(LD)
            if Cn == 0:
                value, grad, bound = f0, g0.astype(LD), ACQ_RTOL * np.abs(f0)
            elif kind == "log_ei":
                value, grad = f0 + L, g0 + dL
                bound = ACQ_RTOL * np.abs(f0) + moments_L + fold["bound"]
            else:
                value, grad = f0 * P, P[:, None] * (g0 + f0[:, None] * dL)
                bound = np.abs(value) * (ACQ_RTOL + moments_L) + fold["bound"]
        elif kind == "log_ei":
            value, grad, bound = L, dL, moments_L + fold["bound"]
        else:
            value, grad, bound = P, P[:, None] * dL, P * moments_L + fold["bound"]
    return dict(value=value, grad=np.asarray(grad, dtype=np.float64), bound=bound, z=zs, L=L,
                dL=np.asarray(dL, dtype=np.float64), floored=floored)


def evaluator(models, thresholds, kind, par, eta):
    """X -> (value (M,), gradient (M, D)) in fp64, refine_oracle.evaluator's protocol (refine_oracle.refine runs on it)"""
    def fn(X):
        r = evaluate(models, thresholds, kind, par, eta, X)
        return np.asarray(r["value"], dtype=np.float64), r["grad"]
    return fn


def pof(models, thresholds, X):
    """the probability of feasibility in fp64"""
    return np.asarray(evaluate(models, thresholds, "ei", 0.0, None, X)["value"], dtype=np.float64)
