"""A plain replay of the regression forest's rule (include/robo_hip.h) in NumPy long double.  It grows no tree of its own: it
takes the device's node tables and checks every node against the rule, with the row set the device's own splits gave it.

Bounds, derived (eps = 2^-52; A = sum w |y_c| over the node's rows; W >= 1 on every side of a split):
  sums       a value of a segmented scan is reached through at most d = 12 + ceil(n / 256) additions (6 shuffle steps, 4 wave
             totals, one carry per tile, and slack for the products' own rounding): |dS| <= e_S = d eps A for S and every S_L;
             the weights are integers and exact.
  score      S_R = S - S_L carries 2 e_S + eps A; s = S_L^2 / W_L + S_R^2 / W_R then moves by at most
             2 A e_S + 2 A (2 e_S + eps A) + 6 eps s.  The chosen and the best score both carry it: the chosen split's exact
             score may fall short of the best exact score by twice that.  (A shift of every y_c by one constant moves every
             score of a node by the same amount, so the oracle uses the device's own ybar, exactly.)
  mean       fl(fl(S / W) + ybar): e_S / W + 2 eps (|S / W| + |mean|).
  variance   with E = eps max |y_c| + e_S / W + 2 eps max |y_c - S / W| the error of one deviation:
             (d + 8) eps var + 2 (sum w |y_c - S / W| / W) E + E^2.
"""
import numpy as np

import bohamiann_oracle as BO

LD, EPS = BO.LD, BO.EPS


def ybar(y):
    s = 0.0
    for v in np.asarray(y, dtype=np.float64):
        s += v
    return s / len(y)


def weights(seed, t, n, n_points, idx=None):
    if idx is None:
        ua, _ = BO.philox(np.arange(n_points), 0, t, 0x52460000, seed)
        idx = np.minimum((ua * float(n)).astype(np.int64), n - 1)
    return np.bincount(np.asarray(idx[t] if np.ndim(idx) == 2 else idx), minlength=n)


def mask(seed, t, node, D, mf):
    if mf >= D:
        return (1 << D) - 1
    perm, out = list(range(D)), 0
    for i in range(mf):
        ua, _ = BO.philox(node, i, t, 0x52460001, seed)
        j = min(i + int(float(ua) * float(D - i)), D - 1)
        perm[i], perm[j] = perm[j], perm[i]
        out |= 1 << perm[i]
    return out


def _best_score(X, w, yc, rows, feats, min_leaf):
    """the best exact score over the admissible splits of `rows` along `feats`, or None"""
    best = None
    for f in feats:
        o = rows[np.lexsort((rows, X[rows, f]))]
        WL, SL = np.cumsum(w[o])[:-1], np.cumsum(w[o] * yc[o])[:-1]
        WR, SR = w[o].sum() - WL, (w[o] * yc[o]).sum() - SL
        ok = (X[o[1:], f] != X[o[:-1], f]) & (WL >= min_leaf) & (WR >= min_leaf)
        if ok.any():
            s = (SL[ok] * SL[ok] / WL[ok] + SR[ok] * SR[ok] / WR[ok]).max()
            best = s if best is None else max(best, s)
    return best


def replay(tree, X, y, w, t, seed, max_features, min_samples_split=2, min_samples_leaf=1, max_depth=2048, eps_purity=1e-8):
    """asserts the rule at every node of one tree -> the largest error / bound seen (score, mean, variance)"""
    n, D = X.shape
    min_split, min_leaf = min_samples_split, min_samples_leaf
    yb, w = ybar(y), np.asarray(w, dtype=LD)
    yc, d = np.asarray(y, dtype=LD) - LD(yb), 12 + -(-n // 256)
    rows, worst, seen = {0: np.flatnonzero(w > 0)}, 0.0, 1
    assert tree["depth"][0] == 0
    for i, nd in enumerate(tree):
        R = rows[i]
        W, S, A = w[R].sum(), (w[R] * yc[R]).sum(), (w[R] * np.abs(yc[R])).sum()
        eS, mc = d * EPS * A, S / W
        mean, dev = mc + LD(yb), yc[R] - mc
        var = (w[R] * dev * dev).sum() / W
        E = EPS * np.abs(yc[R]).max() + eS / W + 2 * EPS * np.abs(dev).max()
        bm = eS / W + 2 * EPS * (abs(mc) + abs(mean)) + LD(1e-300)
        bv = (d + 8) * EPS * var + 2 * (w[R] * np.abs(dev)).sum() / W * E + E * E + LD(1e-300)
        worst = max(worst, float(abs(nd["mean"] - mean) / bm), float(abs(nd["var"] - var) / bv))
        assert nd["weight"] == W and abs(nd["mean"] - mean) <= bm and abs(nd["var"] - var) <= bv, (t, i)
        stopped = W < min_split or nd["depth"] >= max_depth or nd["var"] <= eps_purity
        want_mask = 0 if stopped else mask(seed, t, i, D, max_features)
        assert int(nd["mask"]) == want_mask and (stopped or bin(want_mask).count("1") == min(max_features, D)), (t, i)
        feats = [f for f in range(D) if want_mask >> f & 1]
        best = None if stopped else _best_score(X, w, yc, R, feats, min_leaf)
        if nd["feature"] < 0:
            assert best is None and nd["left"] == nd["right"] == -1, (t, i, "a leaf that could split")
            continue
        f, thr = int(nd["feature"]), nd["threshold"]
        L, Rt = R[X[R, f] <= thr], R[~(X[R, f] <= thr)]
        assert f in feats and nd["left"] == seen and nd["right"] == seen + 1 and len(L) and len(Rt), (t, i)
        assert X[L, f].max() <= thr < X[Rt, f].min() and w[L].sum() >= min_leaf and w[Rt].sum() >= min_leaf, (t, i)
        assert tree["depth"][seen] == tree["depth"][seen + 1] == nd["depth"] + 1
        SL, SR = (w[L] * yc[L]).sum(), (w[Rt] * yc[Rt]).sum()
        s = SL * SL / w[L].sum() + SR * SR / w[Rt].sum()
        bs = 2 * (2 * A * eS + 2 * A * (2 * eS + EPS * A) + 6 * EPS * best) + LD(1e-300)
        worst = max(worst, float((best - s) / bs))
        assert s >= best - bs, (t, i, float(best - s), float(bs))
        rows[seen], rows[seen + 1] = L, Rt
        seen += 2
    assert seen == len(tree)
    return worst


def walk(trees, X):
    """-> every tree's leaf (mean, var) at every row, (T, m) each"""
    mu, v = np.empty((len(trees), len(X))), np.empty((len(trees), len(X)))
    for t, tr in enumerate(trees):
        at = np.zeros(len(X), dtype=np.int64)
        while True:
            f = tr["feature"][at]
            go = f >= 0
            if not go.any():
                break
            left = X[np.arange(len(X)), np.where(go, f, 0)] <= tr["threshold"][at]
            at = np.where(go, np.where(left, tr["left"][at], tr["right"][at]), at)
        mu[t], v[t] = tr["mean"][at], tr["var"][at]
    return mu, v


def moments(mu, v, total_variance):
    """-> the forest's mean and variance before the clip and the bounds on the device's Welford update in tree order: with
    E = (T + 4) eps max |mu_t| on the mean, 4 a E + 4 E^2 + (T + 8) eps var on the variance, a = mean |mu_t - mean|"""
    mu, v, T = np.asarray(mu, dtype=LD), np.asarray(v, dtype=LD), len(mu)
    mean = mu.sum(axis=0) / T
    var = ((mu - mean) ** 2).sum(axis=0) / T + (v.sum(axis=0) / T if total_variance else 0)
    E = (T + 4) * EPS * np.abs(mu).max(axis=0) + LD(1e-300)
    return mean, var, E, 4 * np.abs(mu - mean).mean(axis=0) * E + 4 * E * E + (T + 8) * EPS * var
