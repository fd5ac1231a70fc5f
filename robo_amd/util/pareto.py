"""Two-objective Pareto fronts for minimisation, in the form the expected hypervolume improvement takes them
(include/robo_hip.h, robo_ehvi_*): points strictly below the reference point in both coordinates, mutually non-dominated,
sorted with the first objective strictly ascending and hence the second strictly descending.
"""
import numpy as np

from robo_amd._lib import EHVI_BOX_MAX_BOUNDS, EHVI_BOX_MAX_BOXES


def pareto_front_2d(Y, ref_point):
    """Y (N, 2), ref_point (2,) -> (front (P, 2) sorted as above, indices (P,) into Y).

    Points that are not strictly below ``ref_point`` in both coordinates, points with a NaN, and points another point
    dominates are dropped; among duplicates the lowest index is kept."""
    Y = np.asarray(Y, dtype=np.float64).reshape(-1, 2)
    ref = np.asarray(ref_point, dtype=np.float64).reshape(2)
    inside = np.flatnonzero((Y[:, 0] < ref[0]) & (Y[:, 1] < ref[1]))
    # by the first objective, then the second, then the index: a point enters the front when its second objective is strictly
    # below every earlier one's (an equal first objective with a larger second, and every duplicate, come later and fail)
    order = inside[np.lexsort((inside, Y[inside, 1], Y[inside, 0]))]
    keep, best = [], np.inf
    for j in order:
        if Y[j, 1] < best:
            keep.append(j)
            best = Y[j, 1]
    idx = np.array(keep, dtype=np.int64)
    return Y[idx].reshape(-1, 2).copy(), idx


def hypervolume_2d(front, ref_point):
    """the area that ``front`` (P, 2), sorted as pareto_front_2d returns it, dominates inside ``ref_point``"""
    front = np.asarray(front, dtype=np.float64).reshape(-1, 2)
    ref = np.asarray(ref_point, dtype=np.float64).reshape(2)
    if front.shape[0] == 0:
        return 0.0
    upper = np.concatenate(([ref[1]], front[:-1, 1]))            # b_{i-1}, with b_0 = r2
    return float(np.sum((ref[0] - front[:, 0]) * (upper - front[:, 1])))


def exclusive_contributions_2d(front, ref_point):
    """the hypervolume each point of a sorted front (P, 2) alone adds: (a_{i+1} - a_i) (b_{i-1} - b_i) with the sentinels
    a_{P+1} = r1, b_0 = r2  -> (P,)"""
    front = np.asarray(front, dtype=np.float64).reshape(-1, 2)
    ref = np.asarray(ref_point, dtype=np.float64).reshape(2)
    right = np.concatenate((front[1:, 0], [ref[0]]))
    upper = np.concatenate(([ref[1]], front[:-1, 1]))
    return (right - front[:, 0]) * (upper - front[:, 1])


# ---- any number of objectives (the box form of the expected hypervolume improvement, robo_ehvi_box_*) --------------------------


def pareto_front(Y, ref_point):
    """Y (N, K), ref_point (K,) -> (front (P, K) in lexicographic order of its rows, indices (P,) into Y).

    Points that are not strictly below ``ref_point`` in every coordinate, points with a NaN, and points another point
    dominates are dropped; among duplicates the lowest index is kept."""
    ref = np.asarray(ref_point, dtype=np.float64).reshape(-1)
    K = ref.shape[0]
    Y = np.asarray(Y, dtype=np.float64).reshape(-1, K)
    inside = np.flatnonzero(np.all(Y < ref, axis=1))
    order = inside[np.lexsort((inside,) + tuple(Y[inside, k] for k in range(K - 1, -1, -1)))]
    keep = []
    for j in order:                 # a dominating point, and the first of a run of duplicates, sort earlier
        if not any(np.all(Y[i] <= Y[j]) for i in keep):
            keep.append(j)
    idx = np.array(keep, dtype=np.int64)
    return Y[idx].reshape(-1, K).copy(), idx


def _slabs(R, top):
    """the slab sweep on integer ranks: R (P, K) ranks >= 1 of a point set, top (K,) the rank of the reference point per
    coordinate -> the boxes [(lo_0, hi_0), .., (lo_{K-1}, hi_{K-1})] of a partition of what no point dominates"""
    K = R.shape[1]
    if K == 1:
        return [[(0, int(R[:, 0].min()) if R.shape[0] else int(top[0]))]]
    # a point another one dominates in these K coordinates would only add cuts
    R = np.unique(R, axis=0)
    below = np.all(R[:, None, :] <= R[None, :, :], axis=2)
    R = R[below.sum(axis=0) == 1]
    cuts = np.unique(R[:, -1]).tolist()
    out = []
    for lo, hi in zip([0] + cuts, cuts + [int(top[-1])]):
        for box in _slabs(R[R[:, -1] <= lo, :-1], top[:-1]):
            out.append(box + [(lo, hi)])
            if len(out) > EHVI_BOX_MAX_BOXES:
                raise ValueError("nondominated_boxes: more than %d boxes" % EHVI_BOX_MAX_BOXES)
    return out


def nondominated_boxes(front, ref_point):
    """front (P, K) strictly below ref_point (K,) -> (bounds, boxes) as robo_ehvi_box_* take them: ``bounds`` a list of K
    arrays t_k = (-inf, the distinct coordinates ascending, ref_k), ``boxes`` (B, K, 2) uint16 index pairs (lo, hi) of the
    boxes [t_k[lo], t_k[hi]) that partition the region below ``ref_point`` which no front point dominates.

    A recursive slab sweep: slabs are cut along the last objective between consecutive distinct coordinates; inside the slab
    above coordinate z lies the (K - 1)-dimensional partition for the points whose last coordinate is <= z; K = 1 gives the
    single interval (-inf, min).  ValueError past 258 bounds of an objective or 65 536 boxes."""
    ref = np.asarray(ref_point, dtype=np.float64).reshape(-1)
    K = ref.shape[0]
    front = np.asarray(front, dtype=np.float64).reshape(-1, K)
    if not (np.all(np.isfinite(front)) and np.all(front < ref)):
        raise ValueError("nondominated_boxes: the front must be finite and strictly below the reference point")
    bounds = [np.concatenate(([-np.inf], np.unique(front[:, k]), ref[k:k + 1])) for k in range(K)]
    if max(b.shape[0] for b in bounds) > EHVI_BOX_MAX_BOUNDS:
        raise ValueError("nondominated_boxes: more than %d distinct coordinates in one objective" % (EHVI_BOX_MAX_BOUNDS - 2))
    R = np.stack([np.searchsorted(bounds[k], front[:, k]) for k in range(K)], axis=1).reshape(-1, K)
    top = np.array([b.shape[0] - 1 for b in bounds])
    return bounds, np.array(_slabs(R, top), dtype=np.uint16).reshape(-1, K, 2)


def hypervolume(front, ref_point):
    """the volume that ``front`` (P, K), any point set strictly below ``ref_point`` (the caller's contract: not checked),
    dominates inside it: slabs along the last objective times the (K - 1)-dimensional volume of the points at or below each
    slab -- a Python recursion of about P^(K-1) steps, meant for the fronts of a few dozen points an optimisation run holds"""
    ref = np.asarray(ref_point, dtype=np.float64).reshape(-1)
    K = ref.shape[0]
    front = np.asarray(front, dtype=np.float64).reshape(-1, K)
    if front.shape[0] == 0:
        return 0.0
    if K == 1:
        return float(ref[0] - front[:, 0].min())
    cuts = np.unique(front[:, -1])
    total = 0.0
    for lo, hi in zip(cuts, np.concatenate((cuts[1:], ref[-1:]))):
        total += (hi - lo) * hypervolume(front[front[:, -1] <= lo, :-1], ref[:-1])
    return float(total)


def exclusive_contributions(front, ref_point):
    """the hypervolume each point of ``front`` (P, K) alone adds  -> (P,): P + 1 calls of hypervolume, so about P^K steps"""
    front = np.asarray(front, dtype=np.float64)
    total = hypervolume(front, ref_point)
    return np.array([total - hypervolume(np.delete(front, i, axis=0), ref_point) for i in range(front.shape[0])])
