"""NumPy restatement of the device's gradient refinement (robo_amd/csrc/refine.hip) on the fp64 oracle
(oracle/gp_oracle.py): values and analytic gradients of EI / LogEI / PI / LCB, the selection of the starts, and the
lock-step projected gradient ascent itself.  Test infrastructure only.

All points are in the GP's normalised input space (OracleGP(normalize_input=False) on inputs in [0, 1]^D).
"""
import numpy as np
from scipy.special import erfcx

from oracle import gp_oracle as O

TAIL_T = 16.0            # refine.hip REFINE_TAIL_T: asymptotic series from z <= -16 on
KINDS = ("ei", "log_ei", "pi", "lcb")


def cdf_over_h(z):
    """Phi(z) / (z Phi(z) + phi(z)) the way the device evaluates it: plain quotient for z >= -1, Mills ratio through
    erfcx for -16 < z < -1, 12 terms of the asymptotic series below"""
    z = np.atleast_1d(np.asarray(z, dtype=np.float64))
    out = np.empty_like(z)
    hi = z >= -1.0
    P = O.norm_cdf(z[hi])
    out[hi] = P / (z[hi] * P + O.norm_pdf(z[hi]))
    t = -z[~hi]
    core = t < TAIL_T
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        M = np.sqrt(np.pi / 2.0) * erfcx(t / np.sqrt(2.0))
        r_core = M / (1.0 - t * M)
        u = 1.0 / (t * t)
        num = np.zeros_like(t)
        den = np.zeros_like(t)
        c = 316234143225.0                                   # 23!!
        for n in range(12, 0, -1):
            sgn = -1.0 if n & 1 else 1.0
            num = (num + sgn * c) * u
            den = (den + sgn * c * (2 * n + 1)) * u
            c /= (2 * n - 1)
        r_tail = t * (1.0 + num) / (1.0 + den)
    out[~hi] = np.where(core, r_core, r_tail)
    return out


def cdf_over_h_reference(z, terms=40000):
    """the same quotient for z <= -1 from the continued fraction of the Mills ratio, in extended precision and without
    any cancellation: Phi(-t) / phi(t) = 1 / (t + 1 / (t + 2 / (t + 3 / ...)))  =>  Phi / h = t + 2 / (t + 3 / (t + ...))"""
    t = -np.atleast_1d(np.asarray(z, dtype=np.longdouble))
    assert np.all(t >= 1)
    tail = t.copy()
    for k in range(terms, 1, -1):
        tail = t + np.longdouble(k) / tail
    return tail


def moments(ogp, X, chunk=256):
    """(m, v, dm (M, D), dv (M, D)) of one OracleGP (normalize_input=False, normalize_output=False) at the rows of X:
    OracleGP.predict for the values; the gradients are OracleGP.predictive_gradients' formulas
    (gp_oracle.gp_predictive_gradients: dm = G^T alpha, dv = dself - 2 G^T K^-1 k_*) evaluated for a block of points at
    once for the stationary kernels -- the per-point loop of the oracle takes minutes for the 13 056 trial points of an
    N = 4096 run; tests/test_refine.py pins the two against each other"""
    import scipy.linalg as sla
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    m, v = ogp.predict(X, diag_only=True)
    m, v = np.asarray(m, dtype=np.float64), np.asarray(v, dtype=np.float64)
    if ogp.kind == "fabolas":
        dm, dv = ogp.predictive_gradients(X)
        return m, v, dm[:, :, 0], dv
    theta_k = ogp.theta[:-1]
    amp, met = np.exp(theta_k[0]), np.exp(np.asarray(theta_k[1:], dtype=np.float64))
    alpha = sla.cho_solve((ogp.L, True), ogp.y - ogp.mean, check_finite=False)
    dm, dv = np.empty(X.shape), np.empty(X.shape)
    for c0 in range(0, X.shape[0], chunk):
        Xb = X[c0:c0 + chunk]
        diff = (Xb[:, None, :] - ogp.X[None, :, :]) / np.sqrt(met)
        r2 = np.sum(diff * diff, axis=2)
        if ogp.kind == "matern52":
            t = np.sqrt(5.0 * r2)
            dk = -amp * (5.0 / 6.0) * (1.0 + t) * np.exp(-t)
        else:
            dk = -0.5 * amp * np.exp(-0.5 * r2)
        G = dk[:, :, None] * 2.0 * diff / np.sqrt(met)                      # (B, N, D)
        ks = O.kernel_matrix(ogp.kind, theta_k, Xb, ogp.X)                  # (B, N)
        beta = sla.cho_solve((ogp.L, True), ks.T, check_finite=False)       # (N, B)
        dm[c0:c0 + chunk] = np.einsum("bnd,n->bd", G, alpha)
        dv[c0:c0 + chunk] = -2.0 * np.einsum("bnd,nb->bd", G, beta)
    return m, v, dm, dv


def acq_value_grad(kind, par, eta, m, v, dm, dv):
    """value (M,) and gradient (M, D) of one acquisition from the posterior moments and their gradients: the formulas of
    robo_amd/acquisition_functions/{ei,pi,lcb}.py with derivative=True, and for LogEI
    d log EI = ds / s + (Phi / h)(z) dz,  h = z Phi + phi,  dz = (-dm - z ds) / s"""
    s = np.sqrt(v)
    ds = dv / (2.0 * s)[:, None]
    if kind == "lcb":
        return O.lcb(m, v, par), -(dm - par * ds)
    z = (eta - m - par) / s
    if kind == "ei":
        f = s * (z * O.norm_cdf(z) + O.norm_pdf(z))
        return f, -dm * O.norm_cdf(z)[:, None] + ds * O.norm_pdf(z)[:, None]
    if kind == "pi":
        return O.pi(m, v, eta, par), (-O.norm_pdf(z) / s)[:, None] * (dm + ds * z[:, None])
    if kind == "log_ei":
        dz = (-dm - z[:, None] * ds) / s[:, None]
        return O.log_ei_vec(m, v, eta, par), ds / s[:, None] + cdf_over_h(z)[:, None] * dz
    raise ValueError(kind)


def z_of(ogp, par, eta, X):
    m, v = ogp.predict(X, diag_only=True)
    return (eta - m - par) / np.sqrt(v)


def evaluator(ogps, kind, par, etas):
    """X (M, D) -> (f (M,), g (M, D)): the mean over the oracle GPs (NumPy's axis-0 mean), one GP = the plain value"""
    etas = np.broadcast_to(np.asarray(etas, dtype=np.float64), (len(ogps),))

    def fn(X):
        X = np.atleast_2d(X)
        fs, gs = zip(*[acq_value_grad(kind, par, eta, *moments(g, X)) for g, eta in zip(ogps, etas)])
        return np.mean(np.array(fs), axis=0), np.mean(np.array(gs), axis=0)
    return fn


def select(values, K):
    """rows of the K largest values: descending value, ties by ascending index, NaN never"""
    values = np.asarray(values, dtype=np.float64)
    order = np.argsort(-values, kind="stable")
    order = order[~np.isnan(values[order])]
    return order[:K]


def trial_point(x, g, alpha):
    """-> (y, frozen): the projected unit-length step of length alpha from x, clipped to the box"""
    gp = np.where(((x <= 0.0) & (g < 0.0)) | ((x >= 1.0) & (g > 0.0)), 0.0, g)
    nrm = np.sqrt(np.sum(gp * gp))
    if not (nrm > 0.0 and np.isfinite(nrm)):
        return x.copy(), True
    return np.clip(x + alpha * gp / nrm, 0.0, 1.0), False


def refine(fn, sweep_values, Xc, K, T, step0=0.05):
    """the algorithm of robo_acq_refine_cand on the evaluator fn -> dict(x, value, start_index, f0 (K,), f (K,), X (K, D))"""
    starts = select(sweep_values, K)
    X = np.array(Xc[starts], dtype=np.float64)
    f, g = fn(X)
    f, g = f.copy(), g.copy()
    f0 = f.copy()
    alpha = np.full(len(starts), step0)
    frozen = ~np.isfinite(f)
    for _ in range(T):
        for k in range(len(starts)):
            if frozen[k]:
                continue
            y, stop = trial_point(X[k], g[k], alpha[k])
            if stop:
                frozen[k] = True
                continue
            fy, gy = fn(y[None, :])
            if not np.isfinite(fy[0]):
                frozen[k] = True
            elif fy[0] > f[k]:
                X[k], f[k], g[k] = y, fy[0], gy[0]
                alpha[k] = min(2.0 * alpha[k], 0.5)
            else:
                alpha[k] = alpha[k] / 2.0
    best = int(np.argmax(f))
    return dict(x=X[best], value=f[best], start_index=int(starts[best]), f0=f0, f=f, X=X, starts=starts)
