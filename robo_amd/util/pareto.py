"""Two-objective Pareto fronts for minimisation, in the form the expected hypervolume improvement takes them
(include/robo_hip.h, robo_ehvi_*): points strictly below the reference point in both coordinates, mutually non-dominated,
sorted with the first objective strictly ascending and hence the second strictly descending.
"""
import numpy as np


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
