"""Plain oracle of the tanh network (robo_amd/csrc/mlp.hip): the device's arguments in, np.longdouble throughout, explicit
backpropagation over whole arrays and one Adam step as include/robo_hip.h states it.  It knows nothing of chunks or tiles.
"""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def unpack(p, dim, L, H):
    """the packed vector -> [(W_l (in_l, H), b_l (H))], w_out (H), b_out, and the mask of the weights (not biases)"""
    p, layers, mask, o = np.asarray(p, dtype=LD), [], np.zeros(len(p), dtype=bool), 0
    for l in range(L):
        k = dim if l == 0 else H
        layers.append((p[o:o + k * H].reshape(k, H), p[o + k * H:o + (k + 1) * H]))
        mask[o:o + k * H] = True
        o += (k + 1) * H
    mask[o:o + H] = True
    assert o + H + 1 == len(p)
    return layers, p[o:o + H], p[o + H], mask


def forward(p, dim, L, H, X):
    """-> the activations [a_0 = X, a_1, .., a_L] and f (n,)"""
    layers, w_out, b_out, _ = unpack(p, dim, L, H)
    acts = [np.asarray(X, dtype=LD)]
    for W, b in layers:
        acts.append(np.tanh(acts[-1] @ W + b))
    return acts, acts[-1] @ w_out + b_out


def features(p, dim, L, H, X):
    a = forward(p, dim, L, H, X)[0][-1]
    return np.concatenate((a, np.ones((a.shape[0], 1), dtype=LD)), axis=1)


def loss(p, dim, L, H, X, y, l2=0.0):
    _, w_out, _, mask = unpack(p, dim, L, H)
    e = forward(p, dim, L, H, X)[1] - np.asarray(y, dtype=LD)
    pl = np.asarray(p, dtype=LD)
    return (e @ e) / LD(len(e)) + LD(l2) * (pl[mask] @ pl[mask])


def grad(p, dim, L, H, X, y, l2=0.0):
    """-> the gradient of `loss` and, per entry, the sum of the absolute values of the terms it is made of: the same
    backward pass on absolute values, every row's error taken as |f - y| + sum_j |a_Lj w_out_j| + |b_out| + |y| -- what the
    rounding of the forward pass and of the difference f - y scales with"""
    layers, w_out, b_out, mask = unpack(p, dim, L, H)
    acts, f = forward(p, dim, L, H, X)
    yl, n = np.asarray(y, dtype=LD), LD(len(y))
    out = []
    for absolute in (False, True):
        A = [np.abs(a) for a in acts] if absolute else acts
        e = f - yl
        if absolute:
            e = np.abs(e) + np.abs(acts[-1]) @ np.abs(w_out) + abs(b_out) + np.abs(yl)
        s = 2 * e / n
        g_tail = [A[-1].T @ s, np.array([s.sum()])]
        w, g = np.abs(w_out) if absolute else w_out, []
        delta = s[:, None] * w[None, :] * (1 - acts[-1] ** 2)
        for l in range(L - 1, -1, -1):
            g = [(A[l].T @ delta).ravel(), delta.sum(axis=0)] + g
            if l > 0:
                W = np.abs(layers[l][0]) if absolute else layers[l][0]
                delta = (delta @ W.T) * (1 - acts[l] ** 2)
        g = np.concatenate(g + g_tail)
        pl = np.asarray(p, dtype=LD)
        out.append(g + 2 * LD(l2) * np.where(mask, np.abs(pl) if absolute else pl, 0))
    return out[0], out[1]


def adam_step(p, g, m, v, t, lr):
    """step t (from 1) -> p, m, v, and d p / d g: lr / ((1 - beta1^t) (sqrt(v_hat) + eps)) (1 - beta1) at fixed v"""
    b1, b2, eps = LD(9) / 10, LD(999) / 1000, LD(1) / 10 ** 8
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    denom = np.sqrt(v / (1 - b2 ** t)) + eps
    return p - LD(lr) * (m / (1 - b1 ** t)) / denom, m, v, LD(lr) / denom
