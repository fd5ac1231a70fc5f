"""Plain oracle of ONE generation of the device's differential evolution (robo_amd/csrc/de.hip) as include/robo_hip.h states
it, in NumPy float64: every operation of the rule is rounded once there and here, so the comparison is bit for bit.  It takes
the previous state, the generation's draws and the trial values; it knows nothing of GPs, launches or LDS.
"""
import numpy as np


def idx(u, n):
    return np.minimum((u * float(n)).astype(np.int64), n - 1)


def split_u(u, NP, D):
    """the caller's draws of one (generation, instance) -> u_F, u_a, u_b, u_j (NP,), crossover and repair uniforms (NP, D)"""
    m = u[1:].reshape(NP, 3 + 2 * D)
    return u[0], m[:, 0], m[:, 1], m[:, 2], m[:, 3:3 + D], m[:, 3 + D:]


def philox_draws(philox, seed, g, r, NP, D):
    """the same six from Philox at the stated counters (philox: bohamiann_oracle's)"""
    i, p = np.arange(NP), np.arange((D + 1) // 2)

    def pairs(base):
        return np.stack(philox(g, r, i[:, None], base + p[None, :], seed), axis=2).reshape(NP, -1)[:, :D]
    return (philox(g, r, 0xFFFFFFFF, 0, seed)[0], *philox(g, r, i, 0, seed), philox(g, r, i, 1, seed)[0], pairs(2), pairs(2 ** 31))


def trials(pop, best, draws, f_lo, f_hi, cr):
    """-> F, a, b, jrand, the trial points, the crossover mask, the repair mask"""
    uF, ua, ub, uj, uc, ur = draws
    NP, D = pop.shape
    i = np.arange(NP)
    F = f_lo + uF * (f_hi - f_lo)
    a = idx(ua, NP - 1)
    a = a + (a >= i)
    b = idx(ub, NP - 2)
    b = b + (b >= np.minimum(i, a))
    b = b + (b >= np.maximum(i, a))
    j = idx(uj, D)
    cross = (uc < cr) | (np.arange(D)[None, :] == j[:, None])
    with np.errstate(invalid="ignore"):
        t = np.where(cross, pop[best] + F * (pop[a] - pop[b]), pop)
        rep = ~((t >= 0) & (t <= 1))
    return F, a, b, j, np.where(rep, ur, t), cross, rep


def two_stage(x):
    part = np.zeros(256)
    for k in range(0, len(x), 256):
        part[:len(x[k:k + 256])] += x[k:k + 256]
    s = 128
    while s:
        part[:s] += part[s:2 * s]
        s //= 2
    return part[0]


def select(pop, val, trial, tval, tol, atol):
    """trial None: the start.  -> accept bits, population, values, best, (sum, mean, M2, threshold), code"""
    with np.errstate(invalid="ignore", over="ignore"):
        acc = np.zeros(len(val), dtype=bool) if trial is None else ~np.isnan(tval) & (np.isnan(val) | (tval >= val))
        if trial is not None:
            pop, val = np.where(acc[:, None], trial, pop), np.where(acc, tval, val)
        total = two_stage(val)
        mean = total / len(val)
        m2 = two_stage((val - mean) * (val - mean))
        lim = atol + tol * abs(mean)
        limit = len(val) * (lim * lim)
    code = 2 if trial is not None and np.isnan(tval).all() else int(bool(trial is not None and np.isfinite(val).all() and m2 <= limit))
    return acc, pop, val, 0 if np.isnan(val).all() else int(np.nanargmax(val)), (total, mean, m2, limit), code
