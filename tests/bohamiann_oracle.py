"""Plain oracle of BOHAMIANN's sampler (robo_amd/csrc/bnn.hip) as include/robo_hip.h states it: np.longdouble throughout, the
network's passes from dngo_oracle, and a NumPy restatement of Philox-4x32-10 and Box-Muller.  It knows nothing of tiles,
owners or launches.
"""
import numpy as np

import dngo_oracle as O

LD, EPS = O.LD, O.EPS
MASK = np.uint64(0xFFFFFFFF)


def coefs(lr, n, mdecay):
    """eps2, eps4, c2 formed in fp64 exactly as the host forms them"""
    eps = float(lr) / float(np.sqrt(float(n)))
    eps2 = eps * eps
    return eps2, eps2 * eps2, (2.0 * eps2) * float(mdecay)


def potential(pl, dim, L, H, Xb, yb, n, mu, s, lam):
    pl = np.asarray(pl, dtype=LD)
    p, ell = pl[:-1], pl[-1]
    e = np.asarray(yb, dtype=LD) - O.forward(p, dim, L, H, Xb)[1]
    return (ell + e * e * np.exp(-ell)).sum() / (2 * LD(len(yb))) + ((ell - np.log(LD(mu))) ** 2 / (2 * LD(s)) + LD(lam) / 2 * (p @ p)) / LD(n)


def grad(pl, dim, L, H, Xb, yb, n, mu, s, lam):
    """-> dU / d [p | l] and, per entry, the sum of the absolute values of the terms it is made of"""
    pl = np.asarray(pl, dtype=LD)
    p, ell, B = pl[:-1], pl[-1], LD(len(yb))
    einv = np.exp(-ell)
    g, ga = O.grad(p, dim, L, H, Xb, yb)                     # of sum e^2 / |B|: twice what goes back here, without exp(-l)
    acts, f = O.forward(p, dim, L, H, Xb)
    _, w_out, b_out, _ = O.unpack(p, dim, L, H)
    e, yl = f - np.asarray(yb, dtype=LD), np.asarray(yb, dtype=LD)
    ea = np.abs(e) + np.abs(acts[-1]) @ np.abs(w_out) + abs(b_out) + np.abs(yl)
    gl = (1 - (e @ e) / B * einv) / 2 + (ell - np.log(LD(mu))) / (LD(s) * LD(n))
    gla = LD(0.5) + (ea @ ea) / B * einv / 2 + abs(ell - np.log(LD(mu))) / (LD(s) * LD(n))
    lam_n = LD(lam) / LD(n)
    return np.append(einv / 2 * g + lam_n * p, gl), np.append(einv / 2 * ga + lam_n * np.abs(p), gla)


def velocity(v, g, xi, V, lr, n, mdecay):
    """-> the new v from the NEW V, and eps2 M, sigma, sigma^2 before its clamp, c2 M + eps4 (what sigma^2's rounding scales with)"""
    eps2, eps4, c2 = (LD(c) for c in coefs(lr, n, mdecay))
    v, V, xi = (np.asarray(a, dtype=LD) for a in (v, V, xi))
    M = 1 / (np.sqrt(V) + LD(1e-16))
    raw = c2 * M - eps4
    sig = np.sqrt(np.maximum(raw, LD(1e-16)))
    return v - eps2 * M * g - LD(mdecay) * v + sig * xi, eps2 * M, sig, raw, c2 * M + eps4


def step(row, g, xi, burn, lr, n, mdecay):
    """one step from the state row [p | v | tau | gbar | V] (5, P + 1) -> the next row"""
    p, v, tau, gbar, V = (np.asarray(a, dtype=LD) for a in row)
    if burn:
        r = 1 / (tau + 1)
        tau, gbar, V = tau + 1 - tau * gbar * gbar / V, gbar + r * (g - gbar), V + r * (g * g - V)
    v = velocity(v, g, xi, V, lr, n, mdecay)[0]
    return np.stack((p + v, v, tau, gbar, V))


def philox(c0, c1, c2, c3, seed):
    """Philox-4x32-10 on counters (arrays of one shape) under the 64-bit key -> the two 53-bit uniforms of every block"""
    c = [np.asarray(x, dtype=np.uint64) + np.zeros(np.broadcast(c0, c1, c2, c3).shape, dtype=np.uint64) for x in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & MASK, (k1 + np.uint64(0xBB67AE85)) & MASK
    ua = ((c[0] << np.uint64(32)) | c[1]) >> np.uint64(11)
    ub = ((c[2] << np.uint64(32)) | c[3]) >> np.uint64(11)
    return ua.astype(np.float64) * 2.0 ** -53, ub.astype(np.float64) * 2.0 ** -53


def draw_indices(seed, t, chain, batch, n):
    ua, _ = philox(t & 0xFFFFFFFF, t >> 32, chain, 0x80000000 + np.arange(batch), seed)
    return np.minimum((ua * float(n)).astype(np.int64), n - 1).astype(np.int32)


def draw_normals(seed, t, chain, count):
    """-> xi (count,) in long double and its radius sqrt(-2 log(1 - u1)) (what the device's error scales with)"""
    ua, ub = philox(t & 0xFFFFFFFF, t >> 32, chain, np.arange(count), seed)
    rad = np.sqrt(-2 * np.log(1 - ua.astype(LD)))
    return rad * np.cos(2 * np.arccos(LD(-1)) * ub.astype(LD)), rad


def predict(samples, dim, L, H, X, add_noise=False):
    """-> mean, the between-sample variance (+ the mean noise), every sample's values (S, m)"""
    f = np.stack([O.forward(s[:-1], dim, L, H, X)[1] for s in np.asarray(samples, dtype=LD)])
    var = ((f - f.mean(axis=0)) ** 2).mean(axis=0)
    return f.mean(axis=0), var + (np.exp(np.asarray(samples, dtype=LD)[:, -1]).mean() if add_noise else 0), f
