"""NumPy oracle of the joint Monte-Carlo batch EI with greedy picks (robo_amd/csrc/qei.hip, include/robo_hip.h), in
np.longdouble, on batch_oracle.FrozenGP's conventions (theta, constant mean and output transform frozen; y latent).

The independent statement: the joint posterior of (picks, candidates) is built from the raw inputs -- an extended
precision Cholesky factor of the training gram, V = L^-1 k(X, candidates), Sigma(a, b) = k(a, b) - V_a . V_b -- and the
picks are conditioned on as LATENT values through the Cholesky factor Lpp of Sigma(picks, picks) (pivots floored at
eps / y_std^2): l(x) = Lpp^-1 Sigma(picks, x), residual variance Sigma(x, x) - |l(x)|^2, c_t(x) = l_t(x) sqrt(d_t),
d_t = Lpp[t, t]^2.  In scenario k the picks' values are mean + y_std Lpp z[k], a candidate's mean moves by
y_std l(x) . z[k], and the innermost normal is integrated in closed form (Rao-Blackwell): a term is plain EI.

The normal cdf comes from the fp64 erfc / erfcx (SciPy has no extended one) and everything around it is extended: its
relative error of ~1e-16 is amplified by at most z^2 in EI's cancelling tail, far inside the tests' 1e-7.
"""
import numpy as np
from scipy.special import erfc, erfcx

from oracle import gp_oracle as O

LD = np.longdouble
EPS = O.EPS


def ei_h(z):
    """z Phi(z) + phi(z), the dtype of z kept (np.longdouble or np.float64); the erfcx form below z = -1"""
    z = np.asarray(z)
    zd = z.astype(np.float64)
    phi = np.exp(-z * z / 2) / np.sqrt(2 * np.pi).astype(z.dtype)
    t = -z
    with np.errstate(over="ignore", invalid="ignore"):
        tail = phi * (1 - t * np.sqrt(np.pi / 2).astype(z.dtype) * erfcx(-zd / np.sqrt(2.0)).astype(z.dtype))
        core = z * (0.5 * erfc(-zd / np.sqrt(2.0))).astype(z.dtype) + phi
    return np.where(zd < -1.0, tail, core)


def ei(mean, var, eta):
    s = np.sqrt(var)
    return s * ei_h((eta - mean) / s)


def _chol(K, floor=None):
    n = K.shape[0]
    L = np.zeros_like(K)
    for c in range(n):
        p = K[c, c] - L[c, :c] @ L[c, :c]
        if floor is not None:
            p = max(p, floor) if p == p else p
        L[c, c] = np.sqrt(p)
        if c + 1 < n:
            L[c + 1:, c] = (K[c + 1:, c] - L[c + 1:, :c] @ L[c, :c]) / L[c, c]
    return L


def _forward(L, B):
    B = B.copy()
    for r in range(L.shape[0]):
        B[r] = (B[r] - L[r, :r] @ B[:r]) / L[r, r]
    return B


class JointPosterior(object):
    """latent posterior of the candidates of one FrozenGP, every pair's covariance on demand; dtype np.longdouble (or
    np.float64 for the large case)"""

    def __init__(self, gp, Xc, dtype=LD):
        self.gp, self.Xc, self.dt = gp, np.asarray(Xc, dtype=np.float64), dtype
        k = lambda A, B=None: O.kernel_matrix(gp.kind, gp.theta[:-1], A, B).astype(dtype)      # noqa: E731
        self.k = k
        if dtype is LD:
            K = k(gp.X)
            K[np.diag_indices_from(K)] += LD(np.exp(gp.theta[-1])) + LD(O.JITTER)
            L = _chol(K)
            B = _forward(L, np.column_stack([k(gp.X, self.Xc), (gp.y - gp.mean).astype(dtype)]))
        else:
            import scipy.linalg as sla
            L = O.gp_compute(gp.kind, gp.theta, gp.X)
            B = sla.solve_triangular(L, np.column_stack([k(gp.X, self.Xc), gp.y - gp.mean]), lower=True, check_finite=False)
        self.V, zz = B[:, :-1], B[:, -1]
        self.mu = self.V.T @ zz + dtype(gp.mean)
        self.amp = O.kernel_diag(gp.kind, gp.theta[:-1], self.Xc).astype(dtype)          # k(x, x), latent
        self.var = self.amp - np.sum(self.V * self.V, axis=0)
        self.mean_t = self.mu * dtype(gp.y_std) + dtype(gp.y_mean)
        self.floor = dtype(EPS) / dtype(gp.y_std) ** 2

    def cov(self, p):
        """Sigma(x, x_p) of every candidate x"""
        return self.k(self.Xc, self.Xc[p:p + 1])[:, 0] - self.V.T @ self.V[:, p]

    def condition(self, picks):
        """-> (Lpp (t, t), l (t, m), d (t,), residual latent variance (m,)) after conditioning on the latent values at picks"""
        t = len(picks)
        if t == 0:
            return np.zeros((0, 0), self.dt), np.zeros((0, len(self.mu)), self.dt), np.zeros(0, self.dt), self.var
        C = np.stack([self.cov(p) for p in picks])             # (t, m)
        Spp = C[:, picks].copy()
        Spp[np.diag_indices(t)] = self.var[picks]
        Lpp = _chol(Spp, self.floor)
        l = _forward(Lpp, C)
        return Lpp, l, np.diag(Lpp) ** 2, self.var - np.sum(l * l, axis=0)

    def var_t(self, var_lat):
        v = var_lat * self.dt(self.gp.y_std) ** 2
        return np.where(v < EPS, self.dt(EPS), v)              # np.clip's floor; NaN stays


def scenarios(post, picks, Lpp, z, b0):
    """b^k = min(b0, f^k(picks)),  f^k(picks) = mean_t + y_std Lpp z[k]: (K,)"""
    z = np.asarray(z).astype(post.dt)
    b = np.full(z.shape[0], post.dt(b0))
    if len(picks):
        f = post.mean_t[picks][None, :] + post.dt(post.gp.y_std) * (z[:, :len(picks)] @ Lpp.T)
        b = np.minimum(b, f.min(axis=1))
    return b


def fold(mean_t, var_t, l, z, b, y_std):
    """g(x) = (1 / K) sum_k EI(mean_t(x) + y_std l(x) . z[k], var_t(x), b^k): (m,); the terms (K, m) as well"""
    dt = mean_t.dtype.type
    z = np.asarray(z).astype(dt)
    shift = dt(y_std) * (z[:, :l.shape[0]] @ l)               # (K, m)
    terms = ei(mean_t[None, :] + shift, var_t[None, :], b[:, None])
    return terms.sum(axis=0) / dt(z.shape[0]), terms


class Greedy(object):
    """the rule for ONE or several hyper-parameter samples: value of every candidate given the picks so far"""

    def __init__(self, posts, etas, par, z):
        self.posts, self.par, self.z = posts, par, np.asarray(z, dtype=np.float64)
        self.etas = np.array(np.broadcast_to(etas, (len(posts),)), dtype=np.float64)

    def values(self, picks):
        """-> (marginal values (m,), per-sample state [(Lpp, l, d, var_lat, b)])"""
        acc, state = None, []
        for post, eta in zip(self.posts, self.etas):
            Lpp, l, d, var = post.condition(list(picks))
            b = scenarios(post, list(picks), Lpp, self.z, np.float64(eta) - np.float64(self.par))
            g, _ = fold(post.mean_t, post.var_t(var), l, self.z, b, post.gp.y_std)
            acc = g if acc is None else acc + g
            state.append((Lpp, l, d, var, b))
        return acc / post.dt(len(self.posts)), state

    def run(self, q):
        picks, gains, gaps = [], [], []
        for _ in range(q):
            a, _ = self.values(picks)
            i = O.np_argmax(a.astype(np.float64))
            top = np.sort(a)[-2:] if len(a) > 1 else np.array([a[0], a[0]])
            gaps.append(float((top[1] - top[0]) / abs(top[1])) if len(a) > 1 else 1.0)
            picks.append(int(i))
            gains.append(a[i])
        return picks, gains, gaps


def bounds(post, picks, d, mu_atol, var_rel):
    """what the device's c_t(x), d_t and residual variances may differ from the oracle's by, derived from the base errors
    of the same code path in tests/test_batch_select.py: a posterior covariance entry is off by var_rel k(x, x) (latent
    scale), a mean by mu_atol.  With r_u = sqrt(k / d_u), |c_u(p)| / d_u <= r_u and c_u^2 / d_u^2 <= r_u^2, so
        e_c[t] = base + sum_{u<t} 2 r_u e_c[u]                   (the history term  c_u(x) c_u(p_t) / d_u, both factors)
        e_v[j] = base + sum_{t<j} (2 r_t e_c[t] + r_t^2 e_v[t])  (l^2 = c^2 / d:  2 |c| dc / d + c^2 dd / d^2,  dd = e_v[t])
    per candidate, k the larger of the candidate's and the pick's k(x, x).  -> (e_c (t, m), e_d (t,), e_v (t + 1, m))"""
    f64 = np.float64
    amp = post.amp.astype(f64)
    base = var_rel * amp
    e_c, e_v = [], [base]
    for t, p in enumerate(picks):
        k = np.maximum(amp, amp[p])
        r = [np.sqrt(k / f64(d[u])) for u in range(t + 1)]
        e_c.append(base + sum(2 * r[u] * e_c[u] for u in range(t)))
        e_v.append(base + sum(2 * r[u] * e_c[u] + r[u] ** 2 * e_v[u][picks[u]] for u in range(t + 1)))
    e_d = np.array([e_v[t][p] for t, p in enumerate(picks)])
    return e_c, e_d, e_v


def plain_qei(post, picks, b0, n_draws, rng):
    """E[(b0 - min_t f(p_t))^+] of the picked set by plain Monte Carlo in fp64 -> (estimate, standard error)"""
    Lpp, _, _, _ = post.condition(list(picks))
    zz = rng.standard_normal((n_draws, len(picks)))
    f = post.mean_t[picks].astype(np.float64)[None, :] + post.gp.y_std * (zz @ Lpp.astype(np.float64).T)
    imp = np.maximum(b0 - f.min(axis=1), 0.0)
    return float(imp.mean()), float(imp.std(ddof=1) / np.sqrt(n_draws))
