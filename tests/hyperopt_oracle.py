"""NumPy restatement of the rule of robo_gp_optimize_hypers (robo_amd/csrc/hyperopt.hip, include/robo_hip.h) for
tests/test_hyperopt.py: the objective and its gradient from the fp64 oracle, and the step rule in np.longdouble applied
to the doubles the device stored in its trace."""
import numpy as np

from oracle import gp_oracle as O

L = np.longdouble
ALPHA_MIN = 2.0 ** -40
PAIR_TOL = 1e-10


def objective(kind, X, y, mean_c, prior, theta, h=1e-6):
    """(F, G, G_prior_fd) at theta: oracle log-likelihood + prior.lnprob; oracle gradient with the chain rule on the noise
    entry, the prior's part as a central difference of prior.lnprob (returned separately: it carries the looser tolerance)"""
    assert prior is None or np.isfinite(prior.lnprob(theta))
    theta = np.asarray(theta, dtype=np.float64)
    F = O.gp_log_likelihood(O.gp_compute(kind, theta, X), y, mean_c)
    G = O.gp_grad_log_likelihood(kind, theta, X, y, mean_c).copy()
    G[-1] *= np.exp(theta[-1])
    Gp = np.zeros_like(theta)
    if prior is not None:
        F = F + prior.lnprob(theta)
        for p in range(theta.size):
            e = np.zeros_like(theta)
            e[p] = h
            with np.errstate(invalid="ignore", divide="ignore"):
                lp, l0, lm = prior.lnprob(theta + e), prior.lnprob(theta), prior.lnprob(theta - e)
            Gp[p] = (lp - lm) / (2 * h)
            if not np.isfinite(Gp[p]):          # theta_p on the edge of the support: the one-sided difference inside it
                Gp[p] = (l0 - lm) / h if np.isfinite(lm) else (lp - l0) / h
    return F, G, Gp


def valid(kind, X, y, mean_c, prior, theta):
    """the reference's protocol: inside +-20, the factorisation works, the prior is finite"""
    theta = np.asarray(theta, dtype=np.float64)
    if not np.all(np.abs(theta) <= 20.0):
        return False
    try:
        O.gp_compute(kind, theta, X)
    except np.linalg.LinAlgError:
        return False
    return prior is None or bool(np.isfinite(prior.lnprob(theta)))


def _project(x, v, lower, upper):
    return np.where(((x <= lower) & (v < 0)) | ((x >= upper) & (v > 0)), L(0), v)


def projected_max(x, g, lower, upper):
    return float(np.max(np.abs(_project(x, g, lower, upper))))


def direction(x, g, pairs, lower, upper):
    """-> (d, dropped, no_direction) in longdouble; pairs = [(s, y), ...], oldest first"""
    x, g = x.astype(L), g.astype(L)
    if not pairs:
        nrm = np.sqrt(g @ g)
        d = g / nrm if nrm > 0 else np.zeros_like(g)
    else:
        q = g.copy()
        a, sy = [None] * len(pairs), [None] * len(pairs)
        for i in range(len(pairs) - 1, -1, -1):
            s, yy = pairs[i][0].astype(L), pairs[i][1].astype(L)
            sy[i] = s @ yy
            a[i] = (s @ q) / sy[i]
            q = q - a[i] * yy
        yn = pairs[-1][1].astype(L)
        q = q * (sy[-1] / (yn @ yn))
        for i in range(len(pairs)):
            s, yy = pairs[i][0].astype(L), pairs[i][1].astype(L)
            q = q + (a[i] - (yy @ q) / sy[i]) * s
        d = q
    d = _project(x, d, lower, upper)
    if not (d @ g > 0):
        d = _project(x, g, lower, upper)
        nrm = np.sqrt(d @ d)
        if not (nrm > 0):
            return None, True, True
        return d / nrm, True, False
    return d, False, False


def replay(trace, lower, upper, step0, c1, gtol, history):
    """Every (t, k) of a trace against the rule, on the device's own doubles.  -> dict(final (K, P), values (K),
    status (K), decisions, exempt, max_trial_err): what the call must have returned, how many accept decisions were
    checked / exempt as ties, the largest trial-point error in units of its tolerance."""
    T1, K, W = trace.shape
    P = (W - 3) // 2
    eps = np.finfo(np.float64).eps
    final, values, status = np.zeros((K, P)), np.zeros(K), np.zeros(K, dtype=np.int32)
    decisions = exempt = 0
    worst = 0.0
    for k in range(K):
        z, F, G, a, code = trace[0, k, :P], trace[0, k, P], trace[0, k, P + 1:2 * P + 1], trace[0, k, 2 * P + 1], trace[0, k, -1]
        assert a == step0 and code in (1, 3), (k, a, code)
        assert np.all((z >= lower) & (z <= upper)) or code == 3
        x, f, g, alpha, pairs = z.copy(), F, G.copy(), step0, []
        if code == 3:
            assert np.all(np.isnan(G))
            state, f = 3, np.nan
        else:
            assert np.isfinite(F) and np.all(np.isfinite(G))
            state = 1 if projected_max(x, g, lower, upper) <= gtol else 0
        for t in range(1, T1):
            z, F, G, a, code = trace[t, k, :P], trace[t, k, P], trace[t, k, P + 1:2 * P + 1], trace[t, k, 2 * P + 1], \
                trace[t, k, -1]
            d = None
            if state == 0:
                d, dropped, no_dir = direction(x, g, pairs, lower, upper)
                if dropped:
                    pairs = []
                if no_dir:
                    state = 2
            if state != 0:
                assert code == 2 and np.array_equal(z, x), (t, k, code)          # frozen: the entry repeats the point
                assert F == f or (np.isnan(F) and np.isnan(f)), (t, k, F, f)
                continue
            assert code in (0, 1, 3) and a == alpha, (t, k, code, a, alpha)
            want = np.clip(x.astype(L) + L(alpha) * d, lower, upper)
            tol = 1e-11 * max(1.0, float(np.max(np.abs(x))), float(alpha * np.max(np.abs(d))))
            err = float(np.max(np.abs(z.astype(L) - want)))
            worst = max(worst, err / tol)
            assert err <= tol, (t, k, err, tol)
            assert np.all((z >= lower) & (z <= upper))
            if code == 3:
                assert np.all(np.isnan(G)), (t, k)
            s = z - x
            sg = float(np.sum(s.astype(L) * g.astype(L)))
            decisions += 1
            if code != 3:
                margin = float(L(F) - L(f) - L(c1) * L(sg))
                if abs(margin) <= 256 * eps * (max(1.0, abs(f)) + c1 * float(np.sum(np.abs(s * g)))):
                    exempt += 1
                else:
                    assert (code == 1) == (margin >= 0), (t, k, code, margin)
            if code == 1:
                assert F >= f + min(0.0, c1 * sg) - 256 * eps * max(1.0, abs(f)), (t, k, F, f)     # accepted F does not decrease
                yv = g - G
                sy = float(s.astype(L) @ yv.astype(L))
                if sy > PAIR_TOL * float(np.sqrt(s.astype(L) @ s.astype(L)) * np.sqrt(yv.astype(L) @ yv.astype(L))):
                    pairs.append((s.copy(), yv.copy()))
                    if len(pairs) > history:
                        pairs.pop(0)
                x, f, g, alpha = z.copy(), F, G.copy(), 1.0
                if projected_max(x, g, lower, upper) <= gtol:
                    state = 1
            else:
                alpha = alpha / 2.0
                if alpha < ALPHA_MIN:
                    state = 2
        final[k], values[k], status[k] = x, f, state
    return dict(final=final, values=values, status=status, decisions=decisions, exempt=exempt, max_trial_err=worst)


def winner(values, status):
    """the first start with the largest final F among those that are not dead, or -1"""
    best = -1
    for k in range(len(values)):
        if status[k] != 3 and (best < 0 or values[k] > values[best]):
            best = k
    return best
