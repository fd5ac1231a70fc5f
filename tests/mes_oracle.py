"""NumPy restatement of max-value entropy search as include/robo_hip.h states it (robo_mes_*), for tests/test_mes.py.

For minimisation.  (mu_i, v_i): transformed, floored moments of the candidates, sigma_i = sqrt(v_i).
    F(w)   = sum_i log Phi((w + mu_i) / sigma_i)           (sigma_i == 0: -inf for w < -mu_i, else 0)
    w_lo   = max_i(-mu_i - 8 sigma_i),  w_hi = max_i(-mu_i + 8 sigma_i)
    w_p    : F(w_p) = log p,  p = 1/4, 1/2, 3/4
    b      = (w_1/4 - w_3/4) / (log log(4/3) - log log 4),   a = w_1/2 + b log log 2
    y*_k   = -(a - b log(-log u_k)),  clamped to eta on request
    alpha_i = (1/K) sum_k [gamma phi(gamma) / (2 Phi(gamma)) - log Phi(gamma)],  gamma = (mu_i - y*_k) / sigma_i

F and its roots are taken in np.longdouble (x87 extended precision, 64-bit significand): log Phi is formed from a
positive-term series of erf below |x| = 1 and the continued fraction of erfc above, both to ~1e-19 relative."""
import numpy as np
from scipy.special import log_ndtr

LD = np.longdouble
P = (0.25, 0.5, 0.75)
GUMBEL_DEN = np.log(np.log(4.0 / 3.0)) - np.log(np.log(4.0))
LOGLOG2 = np.log(np.log(2.0))
_SQRT_PI = LD("1.77245385090551602729816748334114518")
_SQRT2 = LD("1.41421356237309504880168872420969808")


def _erf_small(x):
    """erf(x), 0 <= x < 1: (2 / sqrt(pi)) exp(-x^2) sum_n 2^n x^(2n+1) / (2n+1)!!  (all terms positive)"""
    term = x.copy()
    total = x.copy()
    for n in range(1, 90):
        term = term * (2 * x * x) / LD(2 * n + 1)
        total = total + term
    return 2 / _SQRT_PI * np.exp(-x * x) * total


def _log_erfc_large(x):
    """log erfc(x), x >= 1: erfc(x) = exp(-x^2) / (sqrt(pi) (x + (1/2) / (x + 1 / (x + (3/2) / (x + ...)))))"""
    t = x.copy()
    for k in range(600, 0, -1):
        t = x + LD(k) / 2 / t
    return -x * x - np.log(_SQRT_PI * t)


def log_ndtr_ld(z):
    """log Phi(z) in np.longdouble, any finite z (and +-inf)"""
    z = np.atleast_1d(np.asarray(z, dtype=LD))
    out = np.empty_like(z)
    x = np.abs(z) / _SQRT2
    big = x >= 1
    fin = np.isfinite(z)
    m = big & fin
    if m.any():
        le = _log_erfc_large(x[m])
        neg = z[m] < 0
        out[m] = np.where(neg, np.log(LD(0.5)) + le, np.log1p(-np.exp(le) / 2))
    m = ~big
    if m.any():
        e = _erf_small(x[m])
        out[m] = np.log((1 + np.sign(z[m]) * e) / 2)
    out[np.isposinf(z)] = 0
    out[np.isneginf(z)] = -np.inf
    return out


def F_ld(w, mu, var):
    """F(w) in np.longdouble; sigma = sqrt(var) is the fp64 value the device uses, widened"""
    mu, s = np.asarray(mu, dtype=np.float64), np.sqrt(np.asarray(var, dtype=np.float64))
    w = LD(w)
    pos = s > 0
    total = LD(0)
    if pos.any():
        total = np.sum(log_ndtr_ld((w + mu[pos].astype(LD)) / s[pos].astype(LD)))
    if (~pos).any() and np.any(w < -mu[~pos].astype(LD)):
        return -LD(np.inf)
    return total


def F64(w, mu, var):
    """the same in plain fp64 (scipy's log_ndtr), as a sanity reference"""
    mu, s = np.asarray(mu, dtype=np.float64), np.sqrt(np.asarray(var, dtype=np.float64))
    pos = s > 0
    total = float(np.sum(log_ndtr((w + mu[pos]) / s[pos]))) if pos.any() else 0.0
    if (~pos).any() and np.any(w < -mu[~pos]):
        return -np.inf
    return total


def bracket(mu, var):
    mu, s = np.asarray(mu, dtype=np.float64), np.sqrt(np.asarray(var, dtype=np.float64))
    return np.max(-mu - 8 * s), np.max(-mu + 8 * s)


def contract_width(w_lo, w_hi):
    """the widest bracket the search may end with"""
    return max((w_hi - w_lo) * 2.0 ** -46, 4 * np.spacing(max(abs(w_lo), abs(w_hi))))


def root_ld(p, mu, var):
    """w_p by bisection in np.longdouble down to neighbouring numbers"""
    lo, hi = (LD(x) for x in bracket(mu, var))
    logp = np.log(LD(p))
    for _ in range(200):
        mid = lo + (hi - lo) / 2
        if mid <= lo or mid >= hi:
            break
        if F_ld(mid, mu, var) >= logp:
            hi = mid
        else:
            lo = mid
    return lo + (hi - lo) / 2


def gumbel_from_quantiles(w25, w50, w75):
    b = (w25 - w75) / GUMBEL_DEN
    a = w50 + b * LOGLOG2
    return a, b


def draws(a, b, u, clamp=False, eta=0.0):
    y = -(a - b * np.log(-np.log(np.asarray(u, dtype=np.float64))))
    return np.minimum(y, eta) if clamp else y


def sample_min(mu, var, u, clamp=False, eta=0.0):
    """-> (ystar (K,), gumbel (7,)) with the quantiles from the longdouble roots"""
    w_lo, w_hi = bracket(mu, var)
    w = [float(root_ld(p, mu, var)) for p in P]
    a, b = gumbel_from_quantiles(*w)
    return draws(a, b, u, clamp, eta), np.array([w_lo, w_hi, w[0], w[1], w[2], a, b])


def values(mu, var, ystar):
    """alpha (m,): NaN moments give NaN, sigma == 0 gives 0"""
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    ystar = np.asarray(ystar, dtype=np.float64)
    s = np.sqrt(var)
    with np.errstate(all="ignore"):
        gam = (mu[None, :] - ystar[:, None]) / s[None, :]
        lc = log_ndtr(gam)
        r = np.exp(-0.5 * gam ** 2 - 0.9189385332046727 - lc)
        t = np.where(r == 0.0, 0.0, gam * r / 2)
        al = np.sum(t - lc, axis=0) / len(ystar)
    al = np.where(s == 0.0, 0.0, al)
    al[np.isnan(mu) | np.isnan(s)] = np.nan
    return al


def np_argmax(a):
    """np.argmax with NaN maximal, first index on ties (what np.argmax does)"""
    return int(np.argmax(a))
