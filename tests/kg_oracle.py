"""NumPy restatement of the knowledge gradient's envelope rule as include/robo_hip.h states it (robo_kg_*), for
tests/test_kg.py.  For minimisation, over n <= 65 lines a_j + b_j Z:

    KG = min_j a_j - E_Z[min_j (a_j + b_j Z)] = sum_k (B_k - B_{k-1}) f(-|c_k|),   f(-t) = phi(t) - t Phi(-t)

with A = -a, B = -b ordered by (B ascending, A descending, index ascending), equal slopes keeping their first line, and the
upper-envelope stack scan giving the surviving lines and their breakpoints c_k.

Everything is taken in np.longdouble (x87 extended precision, 64-bit significand) on the fp64 inputs the device read.
f is formed without cancellation: below t = sqrt 2 from the positive-term series of erf, above from the continued fraction
of erfc, in which  1 - t Phi(-t) / phi(t) = R / (x + R),  x = t / sqrt 2,  R = (1/2) / (x + 1 / (x + (3/2) / (x + ...))).
"""
import numpy as np

LD = np.longdouble
_SQRT_PI = LD("1.77245385090551602729816748334114518")
_SQRT2 = LD("1.41421356237309504880168872420969808")
_SQRT_2PI = _SQRT_PI * _SQRT2
CUT = 36.0                       # a term with |c| beyond it counts as exactly 0


def f_tail(t):
    """f(-t) = phi(t) - t Phi(-t) for t >= 0 (scalar or array), in np.longdouble; 0 beyond CUT"""
    t = np.atleast_1d(np.asarray(t, dtype=LD))
    out = np.zeros_like(t)
    x = t / _SQRT2
    phi = np.exp(-t * t / 2) / _SQRT_2PI
    big = (x >= 1) & (t <= CUT)
    if big.any():
        xb = x[big]
        u = xb.copy()
        for k in range(600, 1, -1):
            u = xb + LD(k) / 2 / u
        R = LD(1) / 2 / u
        out[big] = phi[big] * R / (xb + R)
    small = x < 1
    if small.any():
        xs = x[small]
        term = xs.copy()
        total = xs.copy()
        for n in range(1, 90):
            term = term * (2 * xs * xs) / LD(2 * n + 1)
            total = total + term
        erf = 2 / _SQRT_PI * np.exp(-xs * xs) * total
        out[small] = phi[small] - t[small] * (1 - erf) / 2
    out[np.isnan(t)] = np.nan
    return out


def lines(s, v, mu, disc_mean, sn2, include_self):
    """(a, b) of one candidate from the device's own doubles: fp64 in, np.longdouble out"""
    s = np.asarray(s, dtype=np.float64).astype(LD)
    sig = np.sqrt(LD(v) + LD(sn2))
    a = np.asarray(disc_mean, dtype=np.float64).astype(LD)
    b = s / sig
    if include_self:
        a = np.append(a, LD(mu))
        b = np.append(b, LD(v) / sig)
    return a, b


def _scan(a, b):
    """the surviving lines of a_j + b_j Z by the stated rule -> (dB_k, |c_k|) arrays, or None for a NaN input"""
    A, B = -np.asarray(a, dtype=LD), -np.asarray(b, dtype=LD)
    if np.isnan(A).any() or np.isnan(B).any():
        return None
    order = sorted(range(len(A)), key=lambda j: (B[j], -A[j], j))
    kept = [j for n, j in enumerate(order) if n == 0 or B[j] != B[order[n - 1]]]
    stack = []                                   # (line, breakpoint from which it is the maximum)
    for i in kept:
        c = LD(-np.inf)
        while stack:
            t, ct = stack[-1]
            c = (A[t] - A[i]) / (B[i] - B[t])
            if not c <= ct:
                break
            stack.pop()
            c = LD(-np.inf)
        stack.append((i, c))
    dB = np.array([B[stack[k][0]] - B[stack[k - 1][0]] for k in range(1, len(stack))], dtype=LD)
    c = np.array([abs(stack[k][1]) for k in range(1, len(stack))], dtype=LD)
    return dB, c


def envelope_batch(line_sets):
    """[(a, b)] -> [(KG, [(dB_k, |c_k|, term_k)])] in np.longdouble; f is evaluated once over all the terms"""
    scans = [_scan(a, b) for a, b in line_sets]
    cs = [sc[1] for sc in scans if sc is not None and len(sc[1])]
    f = f_tail(np.concatenate(cs)) if cs else np.zeros(0, dtype=LD)
    out, pos = [], 0
    for sc in scans:
        if sc is None:
            out.append((LD(np.nan), []))
            continue
        dB, c = sc
        terms, total = [], LD(0)
        for k in range(len(c)):
            term = dB[k] * f[pos + k]
            terms.append((dB[k], c[k], term))
            total = total + term
        pos += len(c)
        out.append((total, terms))
    return out


def envelope(a, b):
    """-> (KG, [(dB_k, |c_k|, term_k)]) of the lines a_j + b_j Z, by the stated rule, in np.longdouble"""
    return envelope_batch([(a, b)])[0]


def bound(terms, b):
    """the value bound of one candidate: 16 eps sum_k term_k (c_k^2 + 1) + 1e-290 max_j |b_j|  -> (bound, the eps sum alone)"""
    eps = LD(np.finfo(np.float64).eps)
    unit = eps * sum((t * (c * c + 1) for _, c, t in terms), LD(0))
    bmax = np.max(np.abs(np.asarray(b, dtype=LD))) if len(b) else LD(0)
    return 16 * unit + LD(1e-290) * bmax, unit


def quadrature(a, b, nodes=2000001, lim=12.0, chunk=8192):
    """KG by plain quadrature of min_j(a_j + b_j z) phi(z): trapezoid rule on [-lim, lim], fp64"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    z = np.linspace(-lim, lim, nodes)
    h = z[1] - z[0]
    total = 0.0
    for i in range(0, nodes, chunk):
        zc = z[i:i + chunk]
        g = (a[:, None] + b[:, None] * zc[None, :]).min(axis=0) * np.exp(-0.5 * zc * zc)
        total += g.sum()
        if i == 0:
            total -= 0.5 * g[0]
        if i + chunk >= nodes:
            total -= 0.5 * g[-1]
    return a.min() - total * h / np.sqrt(2 * np.pi)


def np_argmax(a):
    """np.argmax with NaN maximal (first index)"""
    a = np.asarray(a)
    nan = np.isnan(a)
    return int(np.argmax(nan)) if nan.any() else int(np.argmax(a))
