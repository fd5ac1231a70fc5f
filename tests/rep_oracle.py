"""NumPy restatement of the device's representer chain (robo_amd/csrc/represent.hip) on the fp64 oracle
(oracle/gp_oracle.py): the log-density entropy search samples its representer points from -- the acquisition value inside
the box, -inf outside -- and emcee 2's stretch-move chain around it.  Test infrastructure only.
"""
import numpy as np

from oracle import gp_oracle as O

KINDS = (("ei", 0.0), ("log_ei", 0.0), ("pi", 0.0), ("lcb", 1.0))


def acq_value(kind, par, eta, m, v):
    if kind == "ei":
        s = np.sqrt(v)
        z = (eta - m - par) / s
        return s * (z * O.norm_cdf(z) + O.norm_pdf(z))
    if kind == "log_ei":
        return O.log_ei_vec(m, v, eta, par)
    if kind == "pi":
        return O.pi(m, v, eta, par)
    if kind == "lcb":
        return O.lcb(m, v, par)
    raise ValueError(kind)


def outside(X, lower, upper):
    """InformationGain._proposal_batch's box test, NaN counted as outside"""
    X = np.atleast_2d(X)
    return ~np.all((X >= lower) & (X <= upper), axis=1)


def lnprob(ogp, kind, par, eta, lower, upper):
    """X (M, D) in the caller's input space -> (M,) log-density of the representer proposal"""
    def fn(X):
        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        out = np.full(X.shape[0], -np.inf)
        ins = ~outside(X, lower, upper)
        if np.any(ins):
            m, v = ogp.predict(X[ins], diag_only=True)
            out[ins] = acq_value(kind, par, eta, np.asarray(m, dtype=np.float64), np.asarray(v, dtype=np.float64))
        return out
    return fn


def z_of(ogp, par, eta, X):
    m, v = ogp.predict(np.atleast_2d(X), diag_only=True)
    return (eta - m - par) / np.sqrt(v)


def stretch(c, s, u, a=2.0):
    """emcee 2's proposal, NumPy's operations: z (n,), q (n, D)"""
    z = ((a - 1.0) * u + 1.0) ** 2.0 / a
    return z, c - z[:, None] * (c - s)


def chain(fn, lower, upper, p0, uz, pa, ua, a=2.0):
    """the chain of ensemble_sampler.EnsembleSampler.run_mcmc with the draws given, (T, 2, k / 2) each
    -> dict(pos, lnp, acc, codes (T, 2, k / 2): 0 rejected / 1 accepted / 2 outside, margin (T, 2, k / 2): |lnpdiff - log u|
    relative to the larger magnitude, inf where the decision does not hang on a finite comparison)"""
    p = np.array(p0, dtype=np.float64)
    k, D = p.shape
    half, T = k // 2, uz.shape[0]
    lnp = fn(p)
    acc = np.zeros(k, dtype=np.int64)
    codes = np.zeros((T, 2, half), dtype=np.int64)
    margin = np.full((T, 2, half), np.inf)
    for it in range(T):
        for h in range(2):
            S0, S1 = slice(h * half, (h + 1) * half), slice((1 - h) * half, (2 - h) * half)
            z, q = stretch(p[S1][pa[it, h]], p[S0], uz[it, h], a)
            new = fn(q)
            with np.errstate(invalid="ignore"):
                diff = (D - 1.0) * np.log(z) + new - lnp[S0]
            lu = np.log(ua[it, h])
            take = diff > lu
            fin = np.isfinite(diff)
            margin[it, h, fin] = np.abs(diff[fin] - lu[fin]) / np.maximum(np.abs(diff[fin]), np.abs(lu[fin]))
            codes[it, h] = np.where(outside(q, lower, upper), 2, take.astype(np.int64))
            idx = np.arange(k)[S0][take]
            p[idx], lnp[idx] = q[take], new[take]
            acc[idx] += 1
    return dict(pos=p, lnp=lnp, acc=acc, codes=codes, margin=margin)
