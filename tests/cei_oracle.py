"""NumPy restatement of constrained expected improvement as include/robo_hip.h states it (robo_cei_*), for
tests/test_cei.py.  An objective N(mu_0, s_0^2), C constraints N(mu_k, s_k^2) with thresholds t_k, independent:

    z_k = (t_k - mu_k) / s_k,   L = sum_k log Phi(z_k)  (index order),   PoF = exp(L)
    "ei":  EI(mu_0, v_0, eta, par) * PoF       "log_ei":  LogEI(mu_0, v_0, eta, par) + L       eta None:  PoF resp. L

Everything is taken in np.longdouble (x87 extended precision, 64-bit significand) on the fp64 inputs the device read.
Nothing is formed with cancellation: erfc comes from its continued fraction above x = 1 and from the positive-term series
of erf below (kg_oracle.py's two forms), log Phi on the left directly from the continued fraction's logarithm, and
EI = s f(z) with f(z) = max(z, 0) + f(-|z|), f(-t) without the cut (ehvi_oracle.f_tail).

THE BOUND (bound(), per candidate and per mode), eps = 2^-52.  One eps per rounded operation, the device library's
double-precision functions at their documented worst case (erfc 5, erfcx 4, log, log1p and exp 1 unit in the last place).

One constraint, l = log Phi(z), amp = |z| phi(z) / Phi(z) (how l answers a relative change of z; <= z^2 + 1 on the left,
<= 0.3 on the right):
  * z = (t - mu) / sqrt(v) carries three roundings, relative to z: 3 amp.
  * z < -1:  l = log(erfcx(-z / sqrt 2) / 2) - z^2 / 2.  The scaled argument carries 1.5 (the product and the constant);
    erfcx answers a relative change of its argument by less than 1, and adds 4 of its own: the logarithm's argument is off
    by 5.5 eps relative, the logarithm by 5.5 eps absolute plus its own rounding eps |log|, the square by eps z^2 / 2, the
    difference by eps |l|; |log| + z^2 / 2 = |l| because both terms are negative:  5.5 + 2 |l|.
  * z >= -1:  l = log1p(-q), q = erfc(z / sqrt 2) / 2 = Phi(-z).  erfc answers a relative change of its argument by
    |z| phi / Phi(-z): q is off by (1.5 |z| phi / Phi(-z) + 5) eps relative, log1p by that times q / (1 - q), plus its own
    rounding eps |l|:  1.5 amp + 5 Phi(-z) / Phi(z) + |l|.
  * s == 0: the factor is exact.
  unit_L = sum_k u_k + (C - 1) |L|     (every partial sum is at most |L|: all terms are <= 0)
  |L_dev - L| <= 2 eps unit_L + floor_L   (the multiplier is the count doubled, as the KG and EHVI oracles do)
  floor_L = 2 C 2^-1074: beyond z ~ 38.5 erfc's result Phi(-z) is subnormal, a multiple of 2^-1074 (0 in the end), and so
  is l = -Phi(-z) to first order: an absolute step per constraint, not one relative to l.

  eta None, "log_ei":   2 eps unit_L + floor_L
  eta None, "ei":       |PoF| (2 eps (unit_L + 1) + floor_L) + floor       (exp's rounding; floor: below)
  FOLD, given the objective factor E the device itself reports in its trace:
      "log_ei":         2 eps (unit_L + |E + L|) + floor_L                  (the final addition)
      "ei":             |E PoF| (2 eps (unit_L + 2) + floor_L) + floor      (exp and the product)
  TOTAL, against the oracle's own objective factor: the fold's bound plus what the EI tests grant the objective factor
  (tests/parity_checks.py: EI rtol 1e-10; LogEI rtol 1e-11, 1e-7 where z_0 < -30, assert_logei_close of tests/_tol.py):
      "log_ei":         rtol |LogEI| + 2 eps (unit_L + |value|) + floor_L
      "ei":             |value| (1e-10 + 2 eps (unit_L + 2) + floor_L) + floor
  floor = 2 * 2^-1074 max(1, |E|): where PoF is subnormal (z ~ -38.5 for one constraint) exp and the product are rounded
  to a multiple of 2^-1074, not relative to their size; beyond it both are exactly 0 on the device and below 2^-1074 here.
An infinite oracle value (a violated zero-sigma constraint, LogEI = -inf) must be met exactly, a NaN by a NaN.
"""
import numpy as np

import ehvi_oracle as EO
import kg_oracle as KO

LD = KO.LD
EPS = LD(np.finfo(np.float64).eps)
DOUBLED = 2
EI_RTOL = 1e-10                       # tests/parity_checks.py, EI against the reference's values
LOGEI_RTOL, LOGEI_TAIL_RTOL = 1e-11, 1e-7     # ... LogEI, and its tail z < -30 (tests/_tol.py assert_logei_close)
TINY = LD(2) ** -1074
_LOG2 = np.log(LD(2))
_LOG_SQRT_PI = np.log(KO._SQRT_PI)


def _cf(x):
    """R of the continued fraction erfc(x) = exp(-x^2) / (sqrt(pi) (x + R)), x >= 1"""
    u = x.copy()
    for k in range(600, 1, -1):
        u = x + LD(k) / 2 / u
    return LD(1) / 2 / u


def _erf_small(x):
    """erf(x), 0 <= x < 1, by its positive-term series"""
    term, total = x.copy(), x.copy()
    for n in range(1, 90):
        term = term * (2 * x * x) / LD(2 * n + 1)
        total = total + term
    return 2 / KO._SQRT_PI * np.exp(-x * x) * total


def norm_cdf_pair(z):
    """(log Phi(z), Phi(-z) / Phi(z), phi(z) / Phi(z)) in np.longdouble for an fp64 array z"""
    z = np.atleast_1d(np.asarray(z, dtype=LD))
    x = np.abs(z) / KO._SQRT2
    far = x >= 1
    tail = np.zeros_like(z)                                # Phi(-|z|)
    logtail = np.zeros_like(z)                             # log Phi(-|z|)
    if far.any():
        xf = x[far]
        lt = -xf * xf - _LOG_SQRT_PI - np.log(xf + _cf(xf)) - _LOG2
        logtail[far] = lt
        tail[far] = np.exp(lt)
    if (~far).any():
        t = (1 - _erf_small(x[~far])) / 2
        tail[~far] = t
        logtail[~far] = np.log(t)
    neg = z < 0
    logcdf = np.where(neg, logtail, np.log1p(-tail))
    other = np.where(neg, np.log1p(-tail), logtail)          # log Phi(-z)
    with np.errstate(over="ignore"):
        odds = np.exp(other - logcdf)                        # Phi(-z) / Phi(z) (used on the right only; inf far on the left)
    mills = np.exp(-z * z / 2 - logcdf) / KO._SQRT_2PI       # phi / Phi
    return logcdf, odds, mills


def log_pof(means, vars_, thresholds):
    """constraints' moments (C, m) and thresholds (C,) -> (L, unit_L), (m,) each in np.longdouble; L in index order"""
    means, vars_ = np.asarray(means, dtype=np.float64), np.asarray(vars_, dtype=np.float64)
    assert means.ndim == 2 and means.shape == vars_.shape and means.shape[0] == len(thresholds)
    m = means.shape[1]
    L, units = np.zeros(m, dtype=LD), np.zeros(m, dtype=LD)
    for k, t in enumerate(np.asarray(thresholds, dtype=np.float64)):
        mu, s = means[k].astype(LD), np.sqrt(vars_[k].astype(LD))
        zero = s == 0
        with np.errstate(divide="ignore", invalid="ignore"):
            z = np.where(zero, LD(0), (LD(t) - mu) / np.where(zero, LD(1), s))
        l, odds, mills = norm_cdf_pair(z)
        amp = np.abs(z) * mills
        u = 3 * amp + np.where(z < -1, LD(5.5) + 2 * np.abs(l), LD(1.5) * amp + 5 * odds + np.abs(l))
        l = np.where(zero, np.where(means[k] <= t, LD(0), LD(-np.inf)), l)
        u = np.where(zero, LD(0), u)
        L = L + l
        units = units + u
    with np.errstate(invalid="ignore"):
        units = units + max(len(thresholds) - 1, 0) * np.where(np.isfinite(L), np.abs(L), LD(0))
    return L, units


def objective(mu0, v0, kind, par, eta):
    """(the objective factor in np.longdouble, z_0): EI or LogEI of N(mu0, v0) against eta - par; s_0 == 0: EI is NaN as
    the device's plain form gives it (0 * inf), LogEI takes the reference's branches"""
    mu, s = np.asarray(mu0, dtype=np.float64).astype(LD), np.sqrt(np.asarray(v0, dtype=np.float64).astype(LD))
    d = LD(eta) - mu - LD(par)
    zero = s == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(zero, LD(0), d / np.where(zero, LD(1), s))
        f = np.maximum(z, LD(0)) + EO.f_tail(np.abs(z))
        if kind == "ei":
            return np.where(zero, LD(np.nan), s * f), z
        out = np.log(np.where(zero, LD(1), s)) + np.log(f)
        out = np.where(zero, np.where(d > 0, np.log(np.where(d > 0, d, LD(1))), LD(-np.inf)), out)
        return out, z


def cei_batch(mu0, v0, means, vars_, thresholds, kind, par, eta, obj_dev=None):
    """m candidates -> dict(value, bound, L, unit_L, obj, pof) in np.longdouble.  eta None: no feasible incumbent.
    obj_dev: the objective factor the device reports in its trace -> the FOLD's value and bound on it; otherwise the TOTAL's"""
    mu0, v0 = np.atleast_1d(np.asarray(mu0, dtype=np.float64)), np.atleast_1d(np.asarray(v0, dtype=np.float64))
    thresholds = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    Cn, m = len(thresholds), mu0.shape[0]
    means = np.asarray(means, dtype=np.float64).reshape(Cn, m)
    vars_ = np.asarray(vars_, dtype=np.float64).reshape(Cn, m)
    nan = np.isnan(mu0) | np.isnan(v0) | (v0 < 0) | np.isnan(means).any(axis=0) | np.isnan(vars_).any(axis=0) | \
        (vars_ < 0).any(axis=0)
    safe = lambda a: np.where(nan if a.ndim == 1 else nan[None, :], 1.0, a)       # noqa: E731
    L, unit = log_pof(safe(means), safe(vars_), thresholds)
    floor_L = DOUBLED * Cn * TINY
    with np.errstate(over="ignore", invalid="ignore"):
        pof = np.exp(L)
        if eta is None:
            obj = np.full(m, LD(0) if kind == "log_ei" else LD(1))
            value = L if kind == "log_ei" else pof
            bound = DOUBLED * EPS * unit + floor_L if kind == "log_ei" else \
                np.abs(pof) * (DOUBLED * EPS * (unit + 1) + floor_L) + 2 * TINY
        else:
            if obj_dev is None:
                obj, z0 = objective(safe(mu0), safe(v0), kind, par, eta)
                if kind == "log_ei":
                    grant = np.where(z0 < -30, LD(LOGEI_TAIL_RTOL), LD(LOGEI_RTOL)) * np.abs(obj)
                else:
                    grant = LD(EI_RTOL)
            else:
                obj, grant = np.asarray(obj_dev, dtype=np.float64).astype(LD), LD(0)
            if kind == "log_ei":
                value = obj + L if Cn else obj
                bound = grant + DOUBLED * EPS * (unit + np.abs(value)) + floor_L
            else:
                value = obj * pof if Cn else obj
                bound = np.abs(value) * (grant + DOUBLED * EPS * (unit + 2) + floor_L) + \
                    2 * TINY * np.maximum(LD(1), np.abs(obj))
    value = np.where(nan, LD(np.nan), value)
    return dict(value=value, bound=np.where(np.isfinite(value), bound, LD(0)), L=L, unit_L=unit, obj=obj, pof=pof)


def check(dev, orc):
    """device values against cei_batch's result -> the largest error / bound over the finite values (<= 1 passes);
    infinite and NaN oracle values must be met exactly: returns inf otherwise"""
    dev = np.asarray(dev, dtype=np.float64)
    want, bound = orc["value"], orc["bound"]
    worst = 0.0
    for c in range(dev.shape[0]):
        if np.isnan(want[c]):
            if not np.isnan(dev[c]):
                return np.inf
        elif np.isinf(want[c]):
            if not dev[c] == float(want[c]):
                return np.inf
        else:
            if not np.isfinite(dev[c]):
                return np.inf
            err = abs(LD(dev[c]) - want[c])
            if err > 0:
                worst = max(worst, float(err / bound[c]) if bound[c] > 0 else np.inf)
    return worst


def quadrature(mu0, v0, means, vars_, thresholds, eta, nodes=200001, lim=9.0):
    """E[(eta - y)^+ prod_k 1[c_k <= t_k]] over independent normals by the product trapezoid rule on
    [mu - lim s, mu + lim s]^(C + 1), fp64.  The integrand is a product of one function per axis, so the rule's sum over the
    full grid IS the product of its C + 1 one-dimensional sums, which is how it is formed (a grid of 200001^(C + 1) nodes
    cannot be held) -> (value, the factors the indicators' sums came to, the step h: an indicator's jump costs its factor
    at most one step of the density, 0.4 h)"""
    z = np.linspace(-lim, lim, nodes)
    h = z[1] - z[0]
    w = np.full(nodes, h)
    w[0] = w[-1] = 0.5 * h
    w = w * np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi)
    total = float(np.dot(w, np.maximum(eta - (mu0 + np.sqrt(v0) * z), 0.0)))
    factors = []
    for mu, v, t in zip(means, vars_, thresholds):
        factors.append(float(np.dot(w, (mu + np.sqrt(v) * z <= t).astype(np.float64))))
        total *= factors[-1]
    return total, factors, h


def np_argmax(a):
    return KO.np_argmax(a)
