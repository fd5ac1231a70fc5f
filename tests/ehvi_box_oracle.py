"""The expected hypervolume improvement for K objectives by the ALL-CELLS formula in np.longdouble on the device's own doubles
(tests/test_ehvi_box.py): with the bounds t_k = (-inf, the distinct front coordinates, ref_k) of robo_ehvi_box_*, the sum over
the grid cells whose lower corner no front point dominates of prod_k D_k, D_k = G_k[i + 1] - G_k[i], G = g of
tests/ehvi_oracle.py (not cut at 36).  It knows nothing of the slab sweep: a wrong decomposition cannot agree with it.

Bound of one candidate:  |dev - orc| <= C(K) eps unit + floor,  C(K) = 2 max(9.6, 2 K + 3)  (19.2, 19.2, 22 for K = 2, 3, 4),
    unit = sum over the open cells of  prod_k D_k + sum_k E_k prod_{j != k} D_j,
    E_k = G_k[i + 1] (1 + z_k[i + 1]^2) + G_k[i] (1 + z_k[i]^2)
One rounded g carries 9.6 eps G (1 + z^2) (ehvi_oracle), a box's factor D_k hence 9.6 eps E_k of its two corners, a box term T
to first order 9.6 eps sum_k E_k prod_{j != k} D_j plus, relative to T, the K differences, the K - 1 products and the two
compensated sums (2 eps each whatever B is): 2 K + 3.  A device box is a union of cells -- its D_k the sum of theirs, its E_k
two of their non-negative corner terms -- so the cells' unit is at least the boxes'.  Doubled as in ehvi_oracle.
floor: a g cut at |z| > 36 is short by less than c_k = s_k phi(36) / 36^2, a D_k hence off by at most c_k (the cut bounds are
a prefix):  floor = sum over the open cells of prod_k (D_k + c_k) - prod_k D_k.
"""
import numpy as np

import ehvi_oracle as EO

LD = EO.LD


def bound_factor(K):
    return 2 * max(9.6, 2 * K + 3)


def cells(front, ref):
    """(the bounds per objective, the mask of the grid cells whose lower corner no front point dominates)"""
    ref = np.asarray(ref, dtype=np.float64)
    front = np.asarray(front, dtype=np.float64).reshape(-1, len(ref))
    bounds = [np.concatenate(([-np.inf], np.unique(front[:, k]), ref[k:k + 1])) for k in range(len(ref))]
    lower = np.meshgrid(*[b[:-1] for b in bounds], indexing="ij")
    mask = np.ones(lower[0].shape, dtype=bool)
    for p in front:
        mask &= ~np.all([p[k] <= lower[k] for k in range(len(ref))], axis=0)
    return bounds, mask


def _contract(mask, D):
    """sum over the open cells of prod_k D[k][c, i_k]  -> (m,)"""
    T = np.tensordot(D[-1], mask.astype(LD), axes=(1, mask.ndim - 1))
    for Dk in D[-2::-1]:
        T = np.einsum("c...j,cj->c...", T, Dk)
    return T


def ehvi_batch(means, variances, front, ref):
    """moments (K, m) -> (EHVI, unit, floor), (m,) each, in np.longdouble; a NaN moment or negative variance: (NaN, 0, 0)"""
    means, variances = np.asarray(means, dtype=np.float64), np.asarray(variances, dtype=np.float64)
    nan = np.any(np.isnan(means) | np.isnan(variances) | (variances < 0), axis=0)
    means, variances = np.where(nan, 1.0, means), np.where(nan, 1.0, variances)
    bounds, mask = cells(front, ref)
    D, E, Dc = [], [], []
    for k, b in enumerate(bounds):
        s = np.sqrt(variances[k].astype(LD))
        G, z = EO.g(b, means[k], s)
        W = G * (1 + z * z)
        D.append(G[:, 1:] - G[:, :-1])
        E.append(W[:, 1:] + W[:, :-1])
        Dc.append(D[-1] + (s * EO._PHI_CUT)[:, None])
    total = _contract(mask, D)
    unit = total + sum(_contract(mask, D[:k] + [E[k]] + D[k + 1:]) for k in range(len(D)))
    floor = np.maximum(_contract(mask, Dc) - total, 0)
    total[nan], unit[nan], floor[nan] = np.nan, 0, 0
    return total, unit, floor


def bound(K, unit, floor):
    return LD(bound_factor(K)) * LD(np.finfo(np.float64).eps) * unit + floor
