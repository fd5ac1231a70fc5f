"""The truncated Gaussian mixture of include/robo_hip.h ("Parzen estimators") in np.longdouble, for tests/test_tpe.py: the
direct form e_j = c_j - 0.5 sum ((x - mu) / h)^2 (never the expansion), erfc by SciPy (fp64: its own 2 ulp are in the bounds), a
two-pass logsumexp.  eps = 2^-52.

Bound on c'_j and psi_j (``terms``).  psi: mu - centre, h h, 1 / (h h), the product: 4 roundings -> 5 eps |psi|.  c': the
device adds 3 D + 2 terms and D squares, every partial sum at most A = the sum of the absolute terms -> (4 D + 3) eps A; every
term is 2-ulp libm or at most 6 roundings -> 6 eps A; sum w in index order: n eps; Z = 1 - (erfc + erfc) / 2 with arguments of
3 roundings: |x erfc'(x)| <= 0.49, so 1.5 + 2 eps per erfc on the device and 2 eps here -> 8 eps / Z per dimension in log Z.
    |c' - oracle| <= eps ((4 D + 9) A + n + 8 sum_d 1 / Z_d)

Bound on log p(x) from the device's own (c', psi) (``sweep``).  e_j = c' + phi . psi is a dot product of 2 D terms started at
c', and the device's phi squares t once: delta_j = (2 D + 2) eps (|c'_j| + sum |phi_k psi_jk|).  Logsumexp is 1-Lipschitz in
the maximum norm and a component 40 below the largest weighs e^-40 < eps / 50: the e_j contribute max over the components
within 40 of the maximum of delta_j, plus n e^-40 max_j delta_j.  The sum itself: a term's exp carries 2 ulp and its argument
e - max <= 40 half an ulp of 40 -> 23 eps; a lane group joins n / 16 blocks in sequence, each join one exp (2), one product,
one sum -> 4 n / 16; the tree of four groups 6; the log 2 (1 + log n); the final sum |log p|.
    |log p - oracle| <= max_near delta_j + n e^-40 max delta_j + eps (31 + n / 4 + 2 log n + |log p|)
"""
import numpy as np
from scipy.special import erfc

LD = np.longdouble
EPS = 2.0 ** -52


def _mix(lo, hi, mu, h, w):
    mu = np.asarray(mu, dtype=LD)
    h = np.broadcast_to(np.asarray(h, dtype=LD), mu.shape)
    w = np.ones(mu.shape[0], dtype=LD) if w is None else np.asarray(w, dtype=LD)
    return np.asarray(lo, dtype=LD), np.asarray(hi, dtype=LD), mu, h, w


def _c(lo, hi, mu, h, w):
    """-> c_j, the sum of the absolute terms, sum_d 1 / Z_d"""
    rs2 = np.sqrt(LD(0.5))
    Z = LD(1) - (erfc(((mu - lo) / h * rs2).astype(np.float64)).astype(LD) + erfc(((hi - mu) / h * rs2).astype(np.float64)).astype(LD)) / 2
    with np.errstate(divide="ignore"):
        lw = np.log(w)
    per = np.log(h) + LD(0.5) * np.log(2 * LD(np.pi)) + np.log(Z)
    A = np.where(w > 0, np.abs(lw), 0) + abs(np.log(w.sum())) + (np.abs(np.log(h)) + LD(0.5) * np.log(2 * LD(np.pi)) + np.abs(np.log(Z))).sum(axis=1)
    return lw - np.log(w.sum()) - per.sum(axis=1), A, (1 / Z).sum(axis=1)


def terms(lo, hi, mu, h, w=None):
    """-> (c', psi, bound on c', bound on psi)"""
    lo, hi, mu, h, w = _mix(lo, hi, mu, h, w)
    D = mu.shape[1]
    mc = mu - ((lo.astype(np.float64) + hi.astype(np.float64)) / 2.0).astype(LD)          # the centre, rounded once as on the device
    c, A, iz = _c(lo, hi, mu, h, w)
    quad = (mc * mc / (h * h)).sum(axis=1) / 2
    psi = np.concatenate((mc / (h * h), 1 / (h * h)), axis=1)
    return c - quad, psi, EPS * ((4 * D + 9) * (A + quad) + mu.shape[0] + 8 * iz), 5 * EPS * np.abs(psi)


def logpdf(lo, hi, mu, h, w, X):
    """the direct form -> log p (m,) in long double"""
    lo, hi, mu, h, w = _mix(lo, hi, mu, h, w)
    c = _c(lo, hi, mu, h, w)[0]
    z = (np.asarray(X, dtype=LD)[:, None, :] - mu[None]) / h[None]
    return _lse(c[None] - (z * z).sum(axis=2) / 2)


def _lse(e):
    mx = e.max(axis=1)
    return mx + np.log(np.exp(e - mx[:, None]).sum(axis=1))


def sweep(lo, hi, c, psi, X):
    """log p from the device's own (c', psi) -> (log p (m,), bound (m,)); a NaN row gives (NaN, NaN)"""
    D = np.shape(X)[1]
    t = np.asarray(np.asarray(X, dtype=np.float64) - (np.asarray(lo, dtype=np.float64) + np.asarray(hi, dtype=np.float64)) / 2.0, dtype=LD)
    phi, c, psi = np.concatenate((t, -t * t / 2), axis=1), np.asarray(c, dtype=LD), np.asarray(psi, dtype=LD)
    e = c[None] + phi @ psi.T
    live = np.isfinite(c)
    delta = (2 * D + 2) * EPS * (np.abs(c[live])[None] + np.abs(phi) @ np.abs(psi[live]).T)
    lp, n = _lse(e), c.shape[0]
    with np.errstate(invalid="ignore"):
        near = e[:, live] >= e.max(axis=1)[:, None] - 40
    bound = np.where(near, delta, 0).max(axis=1) + n * np.exp(LD(-40)) * delta.max(axis=1) + \
        EPS * (31 + n / 4.0 + 2 * np.log(n) + np.abs(lp))
    return lp, bound
