"""NumPy oracle of the Monte-Carlo entropy search semantics (DESIGN.md "Monte-Carlo entropy search", csrc/igmc.hip).

Every operation that can change a count or a gain is spelled out in the order the device uses: the innovation
a = (sqrt(v + 1e-10) / u) s, V_x = Vb - (s_a s_b) / u, the outcome means Mb + a W_p, the per-outcome entropy as a
sequential sum over b and the gain as a sequential sum over p divided by Np.  The product L z is BLAS's: its rounding
differs from the device's, so a draw whose two smallest values are within NEAR_TIE (relative) may be counted for a
different representer point; ``gains`` reports those draws.
"""
import sys

import numpy as np

NEAR_TIE = 1e-12


def factor(V):
    """mc_part's ladder -> (L, jitter), or (None, the first jitter beyond 1e4)"""
    n = V.shape[0]
    jitter = 0.0
    while True:
        try:
            with np.errstate(all="ignore"):
                return np.linalg.cholesky(V + jitter * np.eye(n)), jitter
        except np.linalg.LinAlgError:
            jitter = 1e-9 if jitter == 0.0 else jitter * 10
            if jitter > 1e4:
                return None, jitter


def pmin_mc(m, V, z):
    """joint_pmin with the draws z (Nf, N) -> (p_min (N,), jitter)"""
    m = np.asarray(m, dtype=np.float64).reshape(-1)
    L, jitter = factor(np.asarray(V, dtype=np.float64))
    if L is None:
        raise np.linalg.LinAlgError("Cholesky decomposition failed.")
    draws = m[:, None] + L.dot(z.T)
    wins = np.bincount(np.argmin(draws, axis=0), minlength=m.shape[0]).astype(np.float64)
    return np.maximum(wins / z.shape[0], 1e-70), jitter


def entropy0(logP, lmb):
    h = 0.0
    for b in range(logP.shape[0]):
        h = h - np.exp(logP[b]) * (logP[b] + lmb[b])
    return h


def gains(s, v, sn2, Mb, Vb, logP, lmb, W, z, ties=True):
    """-> dict(gain (m,), counts (m, Np, Nb), jitter (m,), tie (m, Np, Nf) bool: near-tie draws, all False when
    ``ties`` is off)"""
    s, v = np.atleast_2d(np.asarray(s, dtype=np.float64)), np.asarray(v, dtype=np.float64).reshape(-1)
    Mb, Vb = np.asarray(Mb, dtype=np.float64).reshape(-1), np.asarray(Vb, dtype=np.float64)
    logP, lmb = np.asarray(logP, dtype=np.float64).reshape(-1), np.asarray(lmb, dtype=np.float64).reshape(-1)
    W = np.asarray(W, dtype=np.float64).reshape(-1)
    m, nb, npo, nf = s.shape[0], Mb.shape[0], W.shape[0], z.shape[0]
    h0 = entropy0(logP, lmb)
    out = dict(gain=np.empty(m), counts=np.zeros((m, npo, nb), dtype=np.int64), jitter=np.empty(m),
               tie=np.zeros((m, npo, nf), dtype=bool))
    for c in range(m):
        with np.errstate(all="ignore"):
            u = v[c] - sn2
            sc = np.sqrt(v[c] + 1e-10) / u
            a = sc * s[c]
            Vc = Vb - np.outer(s[c], s[c]) / u
        L, jitter = factor(Vc)
        out["jitter"][c] = jitter
        if L is None:
            out["gain"][c] = -sys.float_info.max
            continue
        y = L.dot(z.T)                                       # (nb, nf)
        mean = Mb[None, :] + a[None, :] * W[:, None]         # (np, nb)
        vals = mean[:, :, None] + y[None, :, :]              # (np, nb, nf)
        idx = np.argmin(vals, axis=1)                        # (np, nf)
        two = np.sort(vals, axis=1)[:, :2, :] if (nb > 1 and ties) else None
        if two is not None:
            out["tie"][c] = np.abs(two[:, 1] - two[:, 0]) <= NEAR_TIE * np.maximum(np.abs(two[:, 0]), np.abs(two[:, 1]))
        for p in range(npo):
            out["counts"][c, p] = np.bincount(idx[p], minlength=nb)
        q = np.maximum(out["counts"][c] / float(nf), 1e-70)   # (np, nb)
        acc = np.zeros(npo)
        for b in range(nb):
            acc = acc + q[:, b] * (np.log(q[:, b]) + lmb[b])
        H = -acc
        g = 0.0
        for p in range(npo):
            g = g + (h0 - H[p])
        g = g / npo
        out["gain"][c] = g if np.isfinite(g) else -sys.float_info.max
    return out
