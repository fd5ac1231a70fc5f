"""NumPy restatement of the two-objective expected hypervolume improvement as include/robo_hip.h states it (robo_ehvi_*),
for tests/test_ehvi.py.  For minimisation, a reference point r and a front (a_i, b_i), i = 1 .. P, sorted with a strictly
ascending and b strictly descending, with the sentinels a_0 = -inf, a_{P+1} = r1, b_0 = r2:

    EHVI = sum_{i=0}^{P} [g(a_{i+1}; mu1, s1) - g(a_i; mu1, s1)] g(b_i; mu2, s2),
    g(b; mu, s) = E[(b - y)^+] = s f((b - mu) / s),   f(z) = phi(z) + z Phi(z) = max(z, 0) + f(-|z|),   s == 0: max(b - mu, 0)

Everything is taken in np.longdouble (x87 extended precision, 64-bit significand) on the fp64 inputs the device read, the
strips summed in index order.  f(-t) is kg_oracle.f_tail up to t = 36 and the same continued fraction beyond it: THE ORACLE
DOES NOT CUT at 36 as the device does, so what the cut costs has to be covered by the bound's floor.

The bound of one candidate (bound()):     |dev - orc| <= C eps unit + floor

    unit  = sum_i [G1hi (1 + z1hi^2) + G1lo (1 + z1lo^2)] G2 + (G1hi - G1lo) G2 (1 + z2^2)

with G* and z* the strip's g values and standardised arguments (z = 0 where s == 0 and at the sentinel a_0).

C from the operation count, one eps per rounded operation.  One g: s = sqrt(v) (1, through z, whose relative error f
amplifies by z f'(z) / f(z) <= 1 + z^2; 1 more through the factor s), b - mu (1), the quotient (1), f(-|z|) in fp64 (3.6 of
its own units eps (t^2 + 1), measured against 60-digit arithmetic: kern_math.h), the addition of max(z, 0) (1), the product
with s (1): 9.6 eps G (1 + z^2).  A strip's term T = (G1hi - G1lo) G2 therefore carries 9.6 eps times the unit's summand,
plus the difference (1), the product (1) and the compensated sum (2 eps of the sum whatever P is) relative to T, which the
summand's second part exceeds: 13.6.  Doubled: C = 28.

floor: f(-t) < phi(t) / t^2, so a g value the device cut at t > 36 is short by less than c_k = s_k phi(36) / 36^2.  The cut
g values of objective 1 are a prefix of the strips; the difference of two of them is off by at most c_1, times G2; a cut
g of objective 2 is off by c_2, times the strip's difference, and the differences sum to g(r1) - 0:

    floor = c_1 sum_i G2_i + c_2 g(r1; mu1, s1) + (P + 1) c_1 c_2          (phi(36) / 36^2 = 2.0e-285)
"""
import numpy as np

import kg_oracle as KO

LD = KO.LD
BOUND_FACTOR = 28
CUT = KO.CUT
_PHI_CUT = np.exp(-LD(CUT) * LD(CUT) / 2) / KO._SQRT_2PI / (LD(CUT) * LD(CUT))


def f_tail(t):
    """f(-t) = phi(t) - t Phi(-t) for t >= 0 in np.longdouble, WITHOUT the cut at 36"""
    t = np.atleast_1d(np.asarray(t, dtype=LD))
    out = KO.f_tail(np.minimum(t, LD(CUT)))
    far = t > CUT
    if far.any():
        tf = t[far]
        x = tf / KO._SQRT2
        u = x.copy()
        for k in range(60, 1, -1):                 # the continued fraction of erfc converges in a few levels out here
            u = x + LD(k) / 2 / u
        R = LD(1) / 2 / u
        out[far] = np.exp(-tf * tf / 2) / KO._SQRT_2PI * R / (x + R)
    out[np.isnan(t)] = np.nan
    return out


def g(b, mu, s):
    """g(b_j; mu_c, s_c) for b (n,) and mu, s (m,) -> (G, z), (m, n) each, in np.longdouble; b = -inf gives (0, 0); s == 0:
    (max(b - mu, 0), 0)"""
    b = np.atleast_1d(np.asarray(b, dtype=np.float64)).astype(LD)[None, :]
    mu = np.atleast_1d(np.asarray(mu, dtype=np.float64)).astype(LD)[:, None]
    s = np.atleast_1d(np.asarray(s, dtype=LD))[:, None]
    d = b - mu
    pos = (s > 0) & np.isfinite(b)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(pos, d / np.where(s > 0, s, LD(1)), LD(0))
    G = s * (np.maximum(z, LD(0)) + f_tail(np.abs(z).ravel()).reshape(z.shape))
    G = np.where(pos, G, np.where(np.isfinite(b), np.maximum(d, LD(0)), LD(0)))
    return G, z


def strips(front, ref):
    """the strips' upper ends a_1 .. a_{P+1} and heights b_0 .. b_P of a sorted front"""
    front = np.asarray(front, dtype=np.float64).reshape(-1, 2)
    ref = np.asarray(ref, dtype=np.float64)
    return np.concatenate((front[:, 0], ref[:1])), np.concatenate((ref[1:], front[:, 1]))


def ehvi_batch(mu1, v1, mu2, v2, front, ref):
    """m candidates -> (EHVI, unit, floor), (m,) each, in np.longdouble; a NaN moment gives (NaN, 0, 0)"""
    mu1, v1, mu2, v2 = (np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (mu1, v1, mu2, v2))
    nan = np.isnan(mu1) | np.isnan(v1) | np.isnan(mu2) | np.isnan(v2)
    mu1, v1, mu2, v2 = (np.where(nan, 1.0, a) for a in (mu1, v1, mu2, v2))
    ahi, b = strips(front, ref)
    s1, s2 = np.sqrt(v1.astype(LD)), np.sqrt(v2.astype(LD))
    G1hi, z1hi = g(ahi, mu1, s1)
    zero = np.zeros((len(mu1), 1), dtype=LD)
    G1lo, z1lo = np.concatenate((zero, G1hi[:, :-1]), axis=1), np.concatenate((zero, z1hi[:, :-1]), axis=1)
    G2, z2 = g(b, mu2, s2)
    terms = (G1hi - G1lo) * G2
    total = np.zeros(len(mu1), dtype=LD)
    for i in range(terms.shape[1]):                               # index order
        total = total + terms[:, i]
    unit = np.sum((G1hi * (1 + z1hi * z1hi) + G1lo * (1 + z1lo * z1lo)) * G2 + terms * (1 + z2 * z2), axis=1)
    c1, c2 = s1 * _PHI_CUT, s2 * _PHI_CUT
    floor = c1 * np.sum(G2, axis=1) + c2 * G1hi[:, -1] + len(b) * c1 * c2
    total[nan], unit[nan], floor[nan] = np.nan, 0, 0
    return total, unit, floor


def ehvi(mu1, v1, mu2, v2, front, ref):
    """one candidate -> (EHVI, unit, floor)"""
    t, u, f = ehvi_batch([mu1], [v1], [mu2], [v2], front, ref)
    return t[0], u[0], f[0]


def bound(unit, floor):
    return BOUND_FACTOR * LD(np.finfo(np.float64).eps) * unit + floor


def hvi(y1, y2, front, ref):
    """the exact hypervolume gain of the points (y1, y2) (arrays) over a sorted front: the area of the strips each dominates"""
    ahi, b = strips(front, ref)
    alo = np.concatenate(([-np.inf], ahi[:-1]))
    y1, y2 = np.asarray(y1, dtype=np.float64)[..., None], np.asarray(y2, dtype=np.float64)[..., None]
    w = np.clip(ahi - np.maximum(alo, y1), 0.0, None)
    w = np.where(np.isfinite(w), w, 0.0)
    return np.sum(w * np.clip(b - y2, 0.0, None), axis=-1)


def quadrature(mu1, v1, mu2, v2, front, ref, nodes=1601, lim=10.0):
    """EHVI by a product trapezoid rule of HVI(y) phi phi over [mu - lim s, mu + lim s]^2, fp64"""
    s1, s2 = np.sqrt(v1), np.sqrt(v2)
    z = np.linspace(-lim, lim, nodes)
    w = np.full(nodes, z[1] - z[0])
    w[0] = w[-1] = 0.5 * (z[1] - z[0])
    w = w * np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi)
    total = 0.0
    for i in range(nodes):
        total += w[i] * float(np.dot(w, hvi(np.full(nodes, mu1 + s1 * z[i]), mu2 + s2 * z, front, ref)))
    return total


def np_argmax(a):
    return KO.np_argmax(a)
