"""The error contract of the three ensemble entry-point families -- gradient refinement (robo_acq_refine_*), greedy batch
selection (robo_acq_batch_*) and max-value entropy search (robo_mes_eval_*), each in its single-model and its marginal
form -- shared by the interpreter run and the MI355X run of tests/test_ensemble_errors.py.

What is pinned: the exception ``_lib.check`` maps every refusal to, the words of the message where a caller can depend on
them, the order in which the checks fire, and that a refused call leaves no stale bits in the candidate handle's flag
word (a valid call on the same handle afterwards reports the flags it reports on a fresh handle).

Shapes: n = 8 training points, dim = 2, m = 16 candidates, S = 2 samples, 4 starts x 1 step, q = 2 picks, K = 2 draws.
"""
import numpy as np
import pytest

from robo_amd import _lib

N, DIM, M, S = 8, 2, 16, 2
N_STARTS, N_STEPS, Q, K = 4, 1, 2, 2
ETA, PAR = 0.1, 0.01
FAMILIES = ("refine", "batch", "mes")


def _gp(ctx, n=N, dim=DIM, kind="matern52", fp32=False, fit=True, seed=0):
    rs = np.random.RandomState(seed)
    X = rs.rand(n, dim)
    g = _lib.DeviceGP(ctx, kind, N, dim)
    g.set_data(X, np.sin(3.0 * X.sum(axis=1)))
    if fp32:
        g.set_precision(True)
    if fit:
        g.fit(np.concatenate([[0.2], np.log(0.4 + 0.1 * np.arange(dim)), [np.log(1e-3)]]), 0.0)
    return g


class Bench(object):
    """the models and the one candidate handle every row of a family works on"""

    def __init__(self, ctx):
        self.ctx = ctx
        self.good = [_gp(ctx, seed=1), _gp(ctx, seed=1)]
        self.unfitted = _gp(ctx, fit=False)
        self.dim3 = _gp(ctx, dim=3)
        self.n7 = _gp(ctx, n=N - 1)
        self.rbf = _gp(ctx, kind="rbf")
        self.fp32 = _gp(ctx, fp32=True)
        rs = np.random.RandomState(7)
        self.Xc = rs.rand(M, DIM)
        self.cand = _lib.Candidates(ctx, self.Xc)
        self.u = rs.uniform(0.05, 0.95, (S, K))

    def close(self):
        self.cand.close()
        for g in self.good + [self.unfitted, self.dim3, self.n7, self.rbf, self.fp32]:
            g.close()

    def call(self, family, gps, marginal, cand=None, **over):
        """one call of the family at the module's shapes -> its flags, as a tuple"""
        cand = self.cand if cand is None else cand
        eta = np.full(len(gps), ETA) if marginal else ETA
        if family == "refine":
            r = _lib.acq_refine(gps, "ei", PAR, eta, cand, n_starts=over.get("n_starts", N_STARTS),
                                n_steps=over.get("n_steps", N_STEPS), step0=over.get("step0", 0.05), marginal=marginal)
            return (r.flags,)
        if family == "batch":
            r = _lib.acq_batch(gps, "ei", PAR, eta, cand, over.get("q", Q), fantasy=over.get("fantasy", "kriging_believer"),
                               marginal=marginal)
            return tuple(int(f) for f in r.flags)
        k = over.get("K", K)
        u = np.full((len(gps), k), 0.5)
        u[:, :min(k, K)] = self.u[:len(gps), :min(k, K)]
        r = _lib.mes_marginal(gps, eta, cand, u if marginal else u[0], marginal=marginal)
        return (r.flags,)


def check_family(ctx, family):
    b = Bench(ctx)
    try:
        _check_family(b, family)
    finally:
        b.close()


def _check_family(b, family):
    ok1, okS = b.good[:1], b.good
    # the flags of a valid call on a FRESH handle: what every valid call after a refusal must report again
    fresh = {}
    for marginal, gps in ((False, ok1), (True, okS)):
        k = _lib.Candidates(b.ctx, b.Xc)
        fresh[marginal] = b.call(family, gps, marginal, cand=k)
        k.close()
        assert b.call(family, gps, marginal) == fresh[marginal]

    def refused(exc, match, gps, marginal, exact=None, **over):
        with pytest.raises(exc, match=match) as e:
            b.call(family, gps, marginal, **over)
        if exact is not None:
            assert type(e.value) is exact, type(e.value)
        for m2, good in ((False, ok1), (True, okS)):       # no stale bits, whichever form comes next
            assert b.call(family, good, m2) == fresh[m2], (family, marginal, m2)
        return str(e.value)

    def not_fitted(gps, marginal, **over):
        if family == "mes":          # its own status (ROBO_BAD_ARGUMENT) and wording
            return refused(ValueError, "no fitted model", gps, marginal, exact=ValueError, **over)
        return refused(Exception, "trained first", gps, marginal, exact=Exception, **over)

    # an unfitted sample: the only one, the first, the last
    not_fitted([b.unfitted], False)
    not_fitted([b.unfitted, b.good[0]], True)
    msg = not_fitted([b.good[0], b.unfitted], True)
    if family == "mes":
        assert "sample 1" in msg
    # a sample whose dim differs from the candidates' (max-value entropy search has no check of its own: the sweep refuses)
    refused(_lib.RoboBadShape, "dim", [b.dim3], False)
    refused(_lib.RoboBadShape, "dim", [b.dim3, b.good[0]], True)
    refused(_lib.RoboBadShape, "dim", [b.good[0], b.dim3], True)
    if family != "mes":
        # samples with different n
        msg = refused(_lib.RoboBadShape, "first sample", [b.good[0], b.n7], True)
        assert "sample 1" in msg and ("n %d" % (N - 1)) in msg
        # the checks run sample by sample: the first offending sample decides
        refused(_lib.RoboBadShape, "dim", [b.dim3, b.unfitted], True)
        not_fitted([b.unfitted, b.dim3], True)
    else:
        b.call(family, [b.good[0], b.n7], True)            # no n check: samples of different n are served
        not_fitted([b.unfitted, b.dim3], True)
    if family == "refine":
        for over in (dict(n_starts=0), dict(n_starts=_lib.REFINE_MAX_STARTS + 1), dict(n_steps=-1), dict(step0=0.0),
                     dict(step0=0.6), dict(step0=float("nan"))):
            for marginal, gps in ((False, ok1), (True, okS)):
                refused(ValueError, "refine: n_starts", gps, marginal, exact=ValueError, **over)
        # the arguments are judged before the samples
        refused(ValueError, "refine: n_starts", [b.unfitted], False, n_starts=0)
        refused(ValueError, "refine: n_starts", [b.good[0], b.dim3], True, step0=0.6)
    if family == "batch":
        for over in (dict(q=0), dict(q=M + 1)):
            for marginal, gps in ((False, ok1), (True, okS)):
                refused(ValueError, "batch selection: q =", gps, marginal, exact=ValueError, **over)
        _lib.FANTASY_KINDS["no_such_fantasy"] = 99          # past the binding's own check of the name
        try:
            for marginal, gps in ((False, ok1), (True, okS)):
                refused(ValueError, "unknown fantasy kind 99", gps, marginal, exact=ValueError, fantasy="no_such_fantasy")
            refused(ValueError, "unknown fantasy kind 99", [b.unfitted], False, fantasy="no_such_fantasy")
        finally:
            del _lib.FANTASY_KINDS["no_such_fantasy"]
        refused(ValueError, "batch selection: q =", [b.unfitted], False, q=0)
        # fp64 covariance entries only
        refused(ValueError, "fp64", [b.fp32], False, exact=ValueError)
        refused(ValueError, "fp64", [b.fp32, b.good[0]], True, exact=ValueError)
        refused(ValueError, "fp64", [b.good[0], b.fp32], True, exact=ValueError)
        refused(ValueError, "fp64", [b.fp32, b.unfitted], True, exact=ValueError)
        # one kernel kind for all samples
        refused(_lib.RoboBadShape, "batch selection: sample 1", [b.good[0], b.rbf], True)
    if family == "refine":
        b.call(family, [b.good[0], b.rbf], True)            # refinement takes samples of different kinds and precisions
        b.call(family, [b.good[0], b.fp32], True)
    if family == "mes":
        for k in (0, _lib.MES_MAX_K + 1):
            for marginal, gps in ((False, ok1), (True, okS)):
                refused(ValueError, "max-value entropy search: K =", gps, marginal, exact=ValueError, K=k)
        # the draws are judged before the samples
        refused(ValueError, "max-value entropy search: K =", [b.unfitted], False, K=0)
        bad_u = b.u.copy()
        bad_u[1, 1] = 1.0
        with pytest.raises(ValueError, match=r"u\[3\]"):
            _lib.mes_marginal([b.unfitted, b.good[0]], np.full(S, ETA), b.cand, bad_u)
        assert b.call(family, okS, True) == fresh[True]
