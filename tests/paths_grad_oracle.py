"""Gradient of a posterior sample path and the descent rule of robo_paths_descend / robo_paths_refine_cand
(include/robo_hip.h) for tests/test_paths_refine.py.

GradPaths is paths_oracle.Paths with gradients(): the same alpha (long-double Cholesky and substitutions), the derivative
of the kernel that cov_oracle.Posterior.gradients uses -- k = amp f(r2): d k / d xs_d = amp f'(r2) 2 (xs_d - xs'_d) with
f' = -(5/6)(1 + t) e^-t (Matern 5/2, t = sqrt(5 r2)) or -f / 2 (RBF) -- and the features' -sin.  dtype=np.float64 is the
plain fp64 model whose deviation from the long-double oracle the gradient bound is built on.

trial_point / replay / descend restate the rule in np.float64 scalars, one rounding per operation, in the order the header
states: what the device must reproduce bit for bit from its own stored doubles."""
import numpy as np

import paths_oracle as PO

LD = PO.LD


class GradPaths(PO.Paths):

    def gradients(self, Xcs, inv_sqrt_metric=None):
        """d f_s / d x (S, m, D) at scaled candidate rows, output transform applied.  inv_sqrt_metric (D,) = d xs_d / d x_d:
        the gradient in the UNSCALED input space; None: in the scaled one."""
        T = np.dtype(self.dtype).type
        A, B = np.asarray(Xcs).astype(self.dtype), np.asarray(self.Xs).astype(self.dtype)
        om, ph = np.asarray(self.omega).astype(self.dtype), np.asarray(self.phase).astype(self.dtype)
        diff = A[:, None, :] - B[None, :, :]                                  # (m, N, D)
        r2 = np.sum(diff * diff, axis=2)
        if self.kind == "matern52":
            t = np.sqrt(T(5) * r2)
            df = -(T(5) / T(6)) * (T(1) + t) * np.exp(-t)
        elif self.kind == "rbf":
            df = T(-0.5) * np.exp(T(-0.5) * r2)
        else:
            raise ValueError(self.kind)
        coef = T(self.amp) * df * T(2)                                         # (m, N)
        F = om.shape[0]
        fscale = np.sqrt(T(2) * T(self.amp) / T(F))
        s = -fscale * np.sin(A @ om.T + ph[None, :])                           # (m, F)
        g = np.empty((self.w.shape[0],) + A.shape, dtype=self.dtype)
        for p in range(self.w.shape[0]):
            g[p] = (s * self.w[p][None, :]) @ om + np.sum((coef * self.alpha[p][None, :])[:, :, None] * diff, axis=1)
        g = g * self.y_std
        if inv_sqrt_metric is not None:
            g = g * np.asarray(inv_sqrt_metric, dtype=np.float64).astype(self.dtype)[None, None, :]
        return g


# ---- the descent rule, one rounding per operation -------------------------------------------------------------------------------
def trial_point(x, g, alpha):
    """-> (y, frozen): the projected unit step of length alpha against g from x, clipped to the box; bit for bit the
    device's: |g_proj|^2 summed in index order, y_d = x_d - (alpha g_proj_d) / |g_proj|"""
    x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    gp = np.where(((x <= 0.0) & (g > 0.0)) | ((x >= 1.0) & (g < 0.0)), 0.0, g)
    n2 = np.float64(0.0)
    for v in gp:
        n2 = n2 + v * v
    nrm = np.sqrt(n2)
    if not (nrm > 0.0 and np.isfinite(nrm)):
        return x.copy(), True
    y = np.array([xd - (np.float64(alpha) * gd) / nrm for xd, gd in zip(x, gp)], dtype=np.float64)
    return np.minimum(np.maximum(y, 0.0), 1.0), False


def replay(trace, used, step0):
    """every (t, i) of a trace against the rule, on the device's own doubles: the trial point, the step length, the accept
    bit and the code, bit for bit -> (final x (P, D), final f (P,), final g (P, D), steps checked)"""
    T1, P, W = trace.shape
    D = (W - 3) // 2
    xT, fT, gT = np.zeros((P, D)), np.full(P, np.nan), np.zeros((P, D))
    steps = 0
    for i in range(P):
        if not used[i]:
            assert np.all(trace[:, i, -1] == 2), i
            continue
        x, f, g = trace[0, i, :D].copy(), trace[0, i, D], trace[0, i, D + 1:2 * D + 1].copy()
        assert trace[0, i, -1] == (1 if np.isfinite(f) else 3) and trace[0, i, 2 * D + 1] == step0, (i, trace[0, i])
        alpha, frozen = np.float64(step0), not np.isfinite(f)
        for t in range(1, T1):
            y, fy, gy, a_used, code = trace[t, i, :D], trace[t, i, D], trace[t, i, D + 1:2 * D + 1], \
                trace[t, i, 2 * D + 1], trace[t, i, -1]
            steps += 1
            want, stop = trial_point(x, g, alpha)
            if frozen or stop:
                frozen = True
                assert code == 2 and y.tobytes() == x.tobytes(), (t, i, code)
                continue
            assert a_used == alpha, (t, i, a_used, alpha)
            assert y.tobytes() == want.tobytes(), (t, i, y, want)
            if not np.isfinite(fy):
                assert code == 3, (t, i, code)
                frozen = True
                continue
            assert code == (1 if fy < f else 0), (t, i, fy, f, code)
            if fy < f:
                x, f, g, alpha = y.copy(), fy, gy.copy(), min(np.float64(2.0) * alpha, np.float64(0.5))
            else:
                alpha = alpha * np.float64(0.5)
        xT[i], fT[i], gT[i] = x, f, g
    return xT, fT, gT, steps


def descend(fn, x0, T, step0=0.05):
    """the rule on the evaluator fn: x (D,) -> (f, g (D,)) -> (x, f) after T steps"""
    x = np.array(x0, dtype=np.float64)
    f, g = fn(x)
    alpha, frozen = np.float64(step0), not np.isfinite(f)
    for _ in range(T):
        if frozen:
            break
        y, stop = trial_point(x, g, alpha)
        if stop:
            break
        fy, gy = fn(y)
        if not np.isfinite(fy):
            break
        if fy < f:
            x, f, g, alpha = y, fy, gy, min(2.0 * alpha, 0.5)
        else:
            alpha = alpha * 0.5
    return x, f


def group_starts(values, K):
    """robo_paths_refine_cand's selection on one path's sweep values (m,): the best row of every group of 64 consecutive
    rows (first index, NaN maximal), the K groups' bests with the smallest values, ties by ascending row, a group whose best
    is NaN contributes none -> rows (K,), -1 in the unused slots"""
    v = np.asarray(values, dtype=np.float64)
    rows, vals = [], []
    for g0 in range(0, v.shape[0], 64):
        b = g0 + int(np.argmax(-v[g0:g0 + 64]))
        if not np.isnan(v[b]):
            rows.append(b)
            vals.append(v[b])
    rows, vals = np.array(rows, dtype=np.int64), np.array(vals, dtype=np.float64)
    order = np.lexsort((rows, vals))[:K]
    out = np.full(K, -1, dtype=np.int64)
    out[:order.size] = rows[order]
    return out
