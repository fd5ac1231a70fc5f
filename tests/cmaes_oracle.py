"""One generation of the (mu/mu_w, lambda)-CMA-ES that robo_acq_cmaes_cand runs (include/robo_hip.h), in np.longdouble,
with the sum of absolute terms next to every sum: the tests bound the device's error by (terms + a small constant) eps
times that sum.  Nothing of the kernels' structure is in here, and no eigendecomposition."""
import numpy as np

LD = np.longdouble
EPS = np.finfo(np.float64).eps


def constants(n, lam):
    mu = lam // 2
    w = np.log((lam + 1) / 2.0) - np.log(np.arange(1, mu + 1))
    w = w / w.sum()
    me = 1.0 / np.sum(w ** 2)
    cs = (me + 2.0) / (n + me + 5.0)
    c1 = 2.0 / ((n + 1.3) ** 2 + me)
    return dict(mu=mu, w=w, mueff=me, cs=cs, ds=1.0 + 2.0 * max(0.0, np.sqrt((me - 1.0) / (n + 1.0)) - 1.0) + cs,
                cc=(4.0 + me / n) / (n + 4.0 + 2.0 * me / n), c1=c1,
                cmu=min(1.0 - c1, 2.0 * (me - 2.0 + 1.0 / me) / ((n + 2.0) ** 2 + me)),
                chin=np.sqrt(n) * (1.0 - 1.0 / (4.0 * n) + 1.0 / (21.0 * n * n)))


def default_eig_every(n, K):
    return max(1, int(np.floor(1.0 / (10.0 * n * (K["c1"] + K["cmu"])))))


def ranks(values):
    """rank of every sample: descending value, ties by ascending index, NaN last"""
    v = np.asarray(values, dtype=np.float64)
    key = np.where(np.isnan(v), -np.inf, v)
    order = np.lexsort((np.arange(len(v)), -key, np.isnan(v)))
    r = np.empty(len(v), dtype=np.int64)
    r[order] = np.arange(len(v))
    return r


def ask(m, sigma, A, z):
    """-> x (L, D) in the box and the error bound of x, from y = A z"""
    m, A, z = m.astype(LD), A.astype(LD), z.astype(LD)
    terms = z[:, None, :] * A[None, :, :]
    y, ymag = terms.sum(axis=2), np.abs(terms).sum(axis=2)
    x = np.clip(m + LD(sigma) * y, 0.0, 1.0)
    bound = EPS * ((A.shape[0] + 4) * sigma * ymag + 2.0 * (np.abs(m) + sigma * np.abs(y)))
    return x, bound


def repaired(x, m, sigma):
    y = (x.astype(LD) - m.astype(LD)) / LD(sigma)
    return y, 4.0 * EPS * (np.abs(x) + np.abs(m)) / sigma


def tell(K, g, m, sigma, ps, pc, C, Ainv, y, rank, new):
    """the step from the state (m .. Ainv) with the repaired steps y (L, D) and their ranks -> {name: (value, bound)}.
    `new`: the device's own new p_sigma, h_sigma and p_c, which the later quantities are formed from."""
    n, mu, w = len(m), K["mu"], K["w"].astype(LD)
    ysel = y.astype(LD)[np.argsort(rank)[:mu]]
    t = w[:, None] * ysel
    yw, ywmag = t.sum(axis=0), np.abs(t).sum(axis=0)
    e_yw = (mu + 4) * EPS * ywmag
    out = {"m": (np.clip(m.astype(LD) + LD(sigma) * yw, 0.0, 1.0), sigma * e_yw + 2 * EPS * (np.abs(m) + sigma * np.abs(yw)))}
    t = Ainv.astype(LD) * yw[None, :]
    v, e_v = t.sum(axis=1), np.abs(Ainv) @ e_yw + (n + 4) * EPS * np.abs(t).sum(axis=1)
    k = np.sqrt(LD(K["cs"]) * (2 - LD(K["cs"])) * LD(K["mueff"]))
    a = (1 - LD(K["cs"])) * ps.astype(LD)
    out["p_sigma"] = (a + k * v, k * e_v + 4 * EPS * (np.abs(a) + k * np.abs(v)))
    pn = np.sqrt(np.sum(new["p_sigma"].astype(LD) ** 2))
    lhs = pn / np.sqrt(1 - (1 - LD(K["cs"])) ** (2 * (g + 1)))
    rhs = (1.4 + 2.0 / (n + 1.0)) * K["chin"]
    out["h_sigma"] = (1.0 if lhs < rhs else 0.0, abs(lhs - rhs) <= (n + 12) * EPS * lhs)      # (value, undecided)
    arg = LD(K["cs"]) / LD(K["ds"]) * (pn / LD(K["chin"]) - 1)
    s_new = LD(sigma) * np.exp(arg)
    out["sigma"] = (s_new, EPS * s_new * (8 + (n + 8) * K["cs"] / K["ds"] * (pn / K["chin"] + 1)))
    hs = LD(new["h_sigma"])
    k = hs * np.sqrt(LD(K["cc"]) * (2 - LD(K["cc"])) * LD(K["mueff"]))
    a = (1 - LD(K["cc"])) * pc.astype(LD)
    out["p_c"] = (a + k * yw, k * e_yw + 4 * EPS * (np.abs(a) + k * np.abs(yw)))
    p = new["p_c"].astype(LD)
    keep = (1 - LD(K["c1"]) - LD(K["cmu"])) + LD(K["c1"]) * (1 - hs) * LD(K["cc"]) * (2 - LD(K["cc"]))
    t = LD(K["cmu"]) * w[:, None, None] * ysel[:, :, None] * ysel[:, None, :]
    terms = (keep * C.astype(LD), LD(K["c1"]) * np.outer(p, p), t.sum(axis=0))
    out["C"] = (sum(terms), (mu + 8) * EPS * (np.abs(terms[0]) + np.abs(terms[1]) + np.abs(t).sum(axis=0)))
    return out


def sqrt_residuals(C, A, Ainv):
    """max-norm residuals of the defining equations in long double -> (|A A - C|, |A A^-1 - I|)"""
    A, Ainv = A.astype(LD), Ainv.astype(LD)
    return float(np.abs(A @ A - C.astype(LD)).max()), float(np.abs(A @ Ainv - np.eye(len(C), dtype=LD)).max())


def eigh_sqrt(C):
    """the square root and its inverse NumPy's fp64 eigh gives for the same C: the yardstick of the residuals"""
    lam, B = np.linalg.eigh(C)
    return (B * np.sqrt(lam)) @ B.T, (B / np.sqrt(lam)) @ B.T
