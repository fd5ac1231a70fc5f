"""Host replays of the device's own random streams as include/robo_hip.h states them: robo_cand_create_uniform,
robo_cand_create_random and the z = NULL draws of robo_acq_cmaes_cand.  `philox` is bohamiann_oracle.philox (counters and
a 64-bit key -> the two 53-bit uniforms of every block).  The uniforms are exact; the Box-Muller values are np.longdouble.
Nothing here knows how a launch is laid out: an element is a function of (seed, its index)."""
import numpy as np

LD = np.longdouble
EPS = np.finfo(np.float64).eps
PAD = 128                         # the candidate array has m rounded up to a multiple of this many rows
RANDOM_TAG = 0x52425321           # counter word 2 of the random-sampling recipe
TWO_PI = 2 * np.arccos(LD(-1))


def padded(m):
    return (m + PAD - 1) // PAD * PAD


def blocks(philox, seed, total, word2=0):
    """the blocks 0 .. ceil(total / 2) - 1 -> ua, ub (float64, one entry per block)"""
    p = np.arange((total + 1) // 2, dtype=np.uint64)
    return philox(p & np.uint64(0xFFFFFFFF), p >> np.uint64(32), word2, 0, seed)


def uniform(philox, seed, m, dim):
    """robo_cand_create_uniform -> the m x dim points"""
    total = padded(m) * dim
    ua, ub = blocks(philox, seed, total)
    return np.stack([ua, ub], axis=1).ravel()[:total].reshape(-1, dim)[:m]


def box_muller(ua, ub):
    """-> cosine branch, sine branch, rad (long double)"""
    rad = np.sqrt(-2 * np.log(1 - ua.astype(LD)))
    ang = TWO_PI * ub.astype(LD)
    return rad * np.cos(ang), rad * np.sin(ang), rad


def random_sampling(philox, seed, m, dim, n_uniform, loc, scale):
    """robo_cand_create_random -> a dict of m x dim arrays: `branch` (0: a plain uniform, 1: cosine, 2: sine), `point` (the
    uniform, exact, or the clipped Gaussian point), `raw` (the point before the clip) and `bound` (what a float64 evaluation
    of a Gaussian point may be off by: 16 eps rad for the Box-Muller value, scaled, + 2 eps |raw| for the multiply-add
    and the rounding of the result; the clip is 1-Lipschitz).  point, raw: long double"""
    total = padded(m) * dim
    ua, ub = blocks(philox, seed, total, RANDOM_TAG)
    gc, gs, rad = box_muller(ua, ub)

    def halves(a, b):
        return np.stack([a, b], axis=1).ravel()[:total].reshape(-1, dim)[:m]
    u, g, rad = halves(ua, ub).astype(LD), halves(gc, gs), halves(rad, rad)
    e = np.arange(m * dim).reshape(m, dim)
    gauss = (e // dim >= n_uniform)
    raw = np.where(gauss, np.asarray(loc, dtype=LD) + np.asarray(scale, dtype=LD) * g, u)
    bound = np.where(gauss, np.asarray(scale, dtype=LD) * (16 * EPS) * rad + 2 * EPS * np.abs(raw), 0)
    return dict(branch=np.where(gauss, 1 + e % 2, 0), raw=raw, point=np.where(gauss, np.clip(raw, 0, 1), u), bound=bound)


def cmaes_normals(philox, seed, g, r, L, D):
    """the draws of generation g, instance r: block (g, r, sample, pair), cosine to coordinate 2 pair, sine to 2 pair + 1
    -> z (L, D) in long double and the rad each entry's error scales with"""
    pairs = (D + 1) // 2
    ua, ub = philox(g, r, np.arange(L)[:, None], np.arange(pairs)[None, :], seed)
    gc, gs, rad = box_muller(ua, ub)
    return np.stack([gc, gs], axis=2).reshape(L, -1)[:, :D], np.stack([rad, rad], axis=2).reshape(L, -1)[:, :D]
