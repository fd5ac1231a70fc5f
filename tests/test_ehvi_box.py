"""Expected hypervolume improvement for two to four objectives (robo_amd/csrc/ehvi_box.hip, api_ehvi_box.hip, util/pareto.py,
the EHVI class, multi_objective_optimization) against the all-cells formula of tests/ehvi_box_oracle.py on the device's own
doubles, within C(K) eps unit + floor as derived there.  CPU: through the interpreter (tests/hipemu).  -m gpu: the same checks
on the MI355X, plus the fused form at N = 256, D = 4, K = 3, m = 32 773 over a front of 50 points.  The kernel's tile is
TC = 16 candidates by NL = 16 box lanes.  Largest error / bound observed: interpreter 0.16, MI355X 0.16 (NOTES.md; measured once, not asserted).
"""
import itertools
import os
import sys

import numpy as np
import pytest

from robo_amd import _lib
from robo_amd.util.pareto import exclusive_contributions, hypervolume, nondominated_boxes, pareto_front

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ehvi_box_oracle as BO  # noqa: E402
import ehvi_oracle as EO  # noqa: E402
from test_ehvi import _bits, _fit, _theta, emu_ctx, gpu_ctx  # noqa: E402,F401

LD, TC, NL = BO.LD, 16, 16
MS = (401, 4 * TC + 1, TC + 1, TC, TC - 1, 1)
_BOX, _REF3 = (np.zeros(2), np.ones(2)), np.full(3, 2.5)


def _front(K, P, S=12):
    """P mutually non-dominated points with repeated coordinates: compositions of S into K parts, scaled into [0.1, 0.9]"""
    comps = np.array([c for c in itertools.product(range(S + 1), repeat=K) if sum(c) == S], dtype=np.float64)
    pick = np.random.RandomState(10 * K + P).choice(len(comps), P, replace=False)
    return pareto_front(0.1 + 0.8 * comps[pick] / S, np.full(K, 1.1))[0]


def _moments(K, m, seed):
    rs = np.random.RandomState(seed)
    return rs.rand(K, m) * 1.1, (0.055 + rs.rand(K, m) * 1.045) ** 2


def _within(vals, means, variances, front, ref, label, rows=None):
    """the (listed) values against the oracle on the same doubles, within the bound -> the bounds"""
    K = len(ref)
    total, unit, floor = BO.ehvi_batch(means, variances, front, ref)
    for j, c in enumerate(np.arange(len(total)) if rows is None else rows):
        if np.isnan(total[j]):
            assert np.isnan(vals[c]), (label, c)
            continue
        err, lim = abs(LD(vals[c]) - total[j]), BO.bound(K, unit[j], floor[j])
        assert vals[c] >= 0.0 and err <= lim, (label, int(c), vals[c], float(total[j]), float(err), float(lim))
    return BO.bound(K, unit, floor)


@pytest.mark.parametrize("K,P", [(2, 5), (3, 7), (4, 6)])
def test_oracle_and_helpers(K, P):
    """all s_k = 0: the all-cells value is hypervolume(front + {mu}) - hypervolume(front); the boxes tile [0, ref) less the
    dominated part; nondominated_boxes past its limits"""
    front, ref, rs = _front(K, P), np.full(K, 1.1), np.random.RandomState(K)
    bounds, boxes = nondominated_boxes(front, ref)
    assert (K == 2 or min(b.shape[0] for b in bounds) < P + 2) and boxes.dtype == np.uint16
    y = rs.rand(K, 30) * 1.2
    got = np.asarray(BO.ehvi_batch(y, np.zeros_like(y), front, ref)[0], dtype=np.float64)
    want = [hypervolume(np.vstack((front, p[None])), ref) - hypervolume(front, ref) if np.all(p < ref) else 0.0 for p in y.T]
    assert np.max(np.abs(got - want)) <= 1e-14 and max(want) > 0.01
    vol = np.prod([bounds[k][boxes[:, k, 1]] - np.maximum(bounds[k][boxes[:, k, 0]], 0.0) for k in range(K)], axis=0).sum()
    assert abs(vol + hypervolume(front, ref) - 1.1 ** K) <= 1e-14
    t = np.arange(257.0)
    for bad, r in ((np.stack((t, -t), axis=1), [300.0, 1.0]), (np.stack((t, 100 - t, t, t), axis=1)[:100], [300.0] * 4)):
        with pytest.raises(ValueError):                      # 259 bounds in one objective; about 100^3 / 6 boxes
            nondominated_boxes(bad, r)


def _check_values(ctx, K, P):
    """the moments form over a front of P points: every m against the oracle, argmax, flags, a candidate's bits whatever m"""
    front, ref = _front(K, P), np.full(K, 1.1)
    bounds, boxes = nondominated_boxes(front, ref)
    means, variances = _moments(K, MS[0], 100 * K + P)
    full = None
    for m in MS:
        vals, mx, am, fl = _lib.ehvi_box_from_moments(ctx, means[:, :m], variances[:, :m], bounds, boxes)
        full = vals if full is None else full
        assert _bits(vals, full[:m]) and am == EO.np_argmax(vals) and _bits([mx], [vals[am]]) and fl == 0, (K, P, m)
    _within(full, means, variances, front, ref, "K = %d P = %d" % (K, P))
    assert np.mean(full > 0) >= 0.95


def _check_k2(ctx, P):
    """K = 2 with the strips as boxes, B = P + 1 around the lane split: the box kernel and the strip kernel within their bounds"""
    t = np.sort(np.random.RandomState(P).rand(P))
    front, ref = np.stack((t, 1.0 - np.sqrt(t)), axis=1), np.full(2, 1.1)
    bounds, boxes = nondominated_boxes(front, ref)
    means, variances = _moments(2, 70, 7 + P)
    box = _lib.ehvi_box_from_moments(ctx, means, variances, bounds, boxes)[0]
    strip = _lib.ehvi_from_moments(ctx, means[0], variances[0], means[1], variances[1], front, ref)[0]
    b_box = _within(box, means, variances, front, ref, "K = 2 B = %d" % (P + 1))
    _, unit, floor = EO.ehvi_batch(means[0], variances[0], means[1], variances[1], front, ref)
    assert boxes.shape[0] == P + 1 and np.all(np.abs(box.astype(LD) - strip.astype(LD)) <= b_box + EO.bound(unit, floor))


def _check_edges(ctx):
    K, ref, front = 3, np.full(3, 1.1), _front(3, 7)
    bounds, boxes = nondominated_boxes(front, ref)
    means, variances = _moments(K, 50, 5)

    def run(mu, v, flags=0, tag=""):
        vals, mx, am, fl = _lib.ehvi_box_from_moments(ctx, mu, v, bounds, boxes)
        _within(vals, mu, v, front, ref, tag)
        assert fl == flags and am == EO.np_argmax(vals) and (_bits([mx], [vals[am]]) or np.isnan(mx)), (tag, fl)
        return vals
    base = run(means, variances, tag="base")
    for k in range(K):
        mu, v = means.copy(), variances.copy()                # s_k = 0 on, below and above a bound
        mu[k, :3], v[k, :3] = bounds[k][2] + np.array([0.0, -0.01, 0.01]), 0.0
        assert _bits(run(mu, v, _lib.FLAG_ZERO_SIGMA, "s%d = 0" % k)[3:], base[3:])
        mu = means.copy()                                     # a mean 36 s above ref: a factor that is exactly 0
        mu[k] = ref[k] + 36.001 * np.sqrt(variances[k])
        assert _bits(run(mu, variances, tag="36 s above ref"), np.zeros(50))
    assert run(means, np.zeros_like(variances), _lib.FLAG_ZERO_SIGMA, "all s = 0").max() > 0.01
    for arr, bad in ((0, np.nan), (1, np.nan), (1, -1.0)):    # NaN and negative variance: NaN, flagged, the first one wins
        mom = [means.copy(), variances.copy()]
        mom[arr][1, [30, 11]] = bad
        vals, mx, am, fl = _lib.ehvi_box_from_moments(ctx, mom[0], mom[1], bounds, boxes)
        assert np.isnan(vals[[11, 30]]).all() and _bits(np.delete(vals, [11, 30]), np.delete(base, [11, 30]))
        assert fl == _lib.FLAG_NAN and np.isnan(mx) and am == 11
    i = EO.np_argmax(base)                                    # a tie: the first index
    j = 45 if i < 45 else 3
    mu, v = means.copy(), variances.copy()
    mu[:, j], v[:, j] = mu[:, i], v[:, i]
    vals, mx, am, fl = _lib.ehvi_box_from_moments(ctx, mu, v, bounds, boxes)
    assert vals[i] == vals[j] == mx and am == min(i, j)
    rs = np.random.RandomState(8)                             # other batch positions, and m = 1: the same bits
    big = [np.concatenate((rs.rand(K, 21), a[:, ::-1], rs.rand(K, 7) + 0.01), axis=1) for a in (means, variances)]
    assert _bits(_lib.ehvi_box_from_moments(ctx, *big, bounds, boxes)[0][21:71][::-1], base)
    assert _bits(_lib.ehvi_box_from_moments(ctx, means[:, 9:10], variances[:, 9:10], bounds, boxes)[0], base[9:10])
    # the largest table, 4 x 258 bounds, under 257 slabs of an EMPTY front's region: prod_k g(ref_k), as one cell gives it (the
    # slabs' inner corners enter two boxes each with opposite signs and the same other factors)
    wide = [np.concatenate(([-np.inf], np.linspace(0.0, 1.1, _lib.EHVI_BOX_MAX_BOUNDS - 1))) for _ in range(4)]
    slabs = np.zeros((257, 4, 2), dtype=np.uint16)
    slabs[:, :, 1], slabs[:, 0, 0] = 257, np.arange(257)
    slabs[:, 0, 1] = np.arange(1, 258)
    mu, v = _moments(4, TC + 1, 9)
    _within(_lib.ehvi_box_from_moments(ctx, mu, v, wide, slabs)[0], mu, v, np.zeros((0, 4)), np.full(4, 1.1), "limits")


def _check_fused(ctx, N=80, D=3, M=401, P=None, rows=None):
    rs = np.random.RandomState(0)
    X = rs.rand(N, D)
    Y = np.stack((np.sin(3 * X.sum(axis=1)), np.cos(2 * X[:, 0] - X[:, 1]), ((X - 0.4) ** 2).sum(axis=1)), axis=1)
    Y = Y + 0.1 * rs.randn(N, 3)
    gps = [_fit(ctx, kind, _theta(D, ls, noise), X, Y[:, o].copy())
           for o, (kind, ls, noise) in enumerate((("matern52", 0.4, 1e-2), ("rbf", 0.7, 3e-2), ("matern52", 0.9, 1e-2)))]
    ref = Y.max(axis=0) + 0.1
    front = pareto_front(Y, ref)[0] if P is None else Y.min(axis=0) + (_front(3, P, 24) - 0.1) * (ref - 0.05 - Y.min(axis=0)) / 0.8
    bounds, boxes = nondominated_boxes(front, ref)
    cand, other = _lib.Candidates(ctx, rs.rand(M, D)), _lib.Context(0)
    far, wide, raw = _lib.Candidates(other, rs.rand(5, D)), _lib.Candidates(ctx, rs.rand(5, D + 1)), _lib.DeviceGP(ctx, "rbf", N, D)
    g_far = _fit(other, "rbf", _theta(D, 0.5, 1e-2), X, Y[:, 1].copy())
    try:
        ei = gps[0].acq("ei", 0.0, float(Y[:, 0].min()), cand)
        r = gps[0].ehvi_box(gps[1:], cand, bounds, boxes, diagnostics=True)
        assert r.flags == 0 and r.trace.shape == (M, 6) and r.argmax == EO.np_argmax(r.values) and _bits([r.max], [r.values[r.argmax]])
        for o, g in enumerate(gps):                                  # the trace is robo_gp_predict_cand's, bit for bit
            mean, var = g.predict(cand)
            assert _bits(r.trace[:, 2 * o], mean) and _bits(r.trace[:, 2 * o + 1], var)
        tr = r.trace if rows is None else r.trace[rows]
        _within(r.values, tr[:, 0::2].T, tr[:, 1::2].T, front, ref, "fused", rows=rows)
        mom = (r.trace[:, 0::2].T, r.trace[:, 1::2].T)
        vals, mx, am, fl = _lib.ehvi_box_from_moments(ctx, *mom, bounds, boxes)
        assert _bits(vals, r.values) and _bits([mx], [r.max]) and (am, fl) == (r.argmax, r.flags)
        ctx.set_tuning("ws_bytes", 128 * 128 * 8)                    # several passes through a small workspace
        try:
            rp = gps[0].ehvi_box(gps[1:], cand, bounds, boxes)
            assert N > 128 or cand.chunk() == 128
        finally:
            ctx.set_tuning("ws_bytes", None)
        assert _bits(rp.values, r.values) and (rp.max, rp.argmax, rp.flags) == (r.max, r.argmax, r.flags)
        for a, b in zip(ei, gps[0].acq("ei", 0.0, float(Y[:, 0].min()), cand)):      # the plain sweep on these handles: unchanged
            assert _bits([a], [b])
        if rows is not None:
            return

        def refuse(exc, gs=gps, cd=cand, bd=bounds, bx=boxes):       # the status, nothing launched; both entry points
            with pytest.raises(exc):
                gs[0].ehvi_box(gs[1:], cd, bd, bx)
            if gs is gps and cd is cand:
                with pytest.raises(exc):
                    _lib.ehvi_box_from_moments(ctx, *mom, bd, bx)

        def edit(k, j, v):
            return [np.concatenate((b[:j], [v], b[j:][1:])) if o == k else b for o, b in enumerate(bounds)]
        hi, eq = boxes.copy(), boxes.copy()
        hi[-1, 2, 1], eq[0, 1, 0] = bounds[2].shape[0], eq[0, 1, 1]
        for kw in (dict(gs=gps[:1], bd=bounds[:1], bx=boxes[:, :1]),                                     # K = 1, K = 5
                   dict(gs=gps + gps[:2], bd=bounds + bounds[:2], bx=np.concatenate((boxes, boxes[:, :2]), axis=1)),
                   dict(bd=edit(0, 0, -1e300)), dict(bd=edit(1, 1, np.nan)), dict(bd=edit(2, -1, np.inf)),
                   dict(bd=edit(1, 2, bounds[1][1])), dict(bx=hi), dict(bx=eq), dict(bx=boxes[:0]),
                   dict(bd=[np.concatenate((bounds[0], 2.0 + np.arange(258.0)))] + bounds[1:]), dict(bd=[bounds[0][:1]] + bounds[1:]),
                   dict(bx=np.tile(boxes, (_lib.EHVI_BOX_MAX_BOXES // len(boxes) + 1, 1, 1))), dict(cd=far),
                   dict(gs=[gps[0], g_far, gps[2]])):
            refuse(ValueError, **kw)
        refuse(_lib.RoboBadShape, cd=wide)
        with pytest.raises(Exception, match="trained first"):
            gps[0].ehvi_box([raw, gps[2]], cand, bounds, boxes)
        tail = _lib._ehvi_box_tail(bounds, boxes, 3)
        for pos in (0, 2, 3, 4, 5):                                  # a NULL required pointer
            args = [_lib._handles(gps), 3, cand._h] + list(tail[:3])
            args[pos] = None
            assert _lib.lib().robo_ehvi_box_eval_cand(*args, tail[3], None, *_lib._Best().refs, None) == _lib.BAD_ARGUMENT, pos
        assert _bits(gps[0].ehvi_box(gps[1:], cand, bounds, boxes).values, r.values)
    finally:
        for h in [cand, far, wide, raw, g_far, other] + gps:
            h.close()


def _toy3(x):
    x = np.asarray(x, dtype=np.float64)
    return float(np.sum(x ** 2)), float(np.sum((x - 1.0) ** 2)), float(np.sum((x - [1.0, 0.0]) ** 2))


def _check_classes(ctx):
    """EHVI over three GaussianProcess models (fused) and with one GaussianProcessMCMC (moments); the 3-objective front end
    against 8 uniform draws on the same seed"""
    from robo_amd.acquisition_functions import EHVI
    from robo_amd.fmin import multi_objective_optimization
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models import GaussianProcess, GaussianProcessMCMC
    from robo_amd.priors.default_priors import DefaultPrior
    rs = np.random.RandomState(0)
    X, Xc = rs.rand(12, 2), rs.rand(40, 2)
    Y = np.array([_toy3(x) for x in X])
    models = [GaussianProcess(Matern52Kernel(np.array([ls, ls]), ndim=2), noise=1e-3, lower=_BOX[0], upper=_BOX[1],
                              normalize_output=ls == 0.9) for ls in (0.6, 0.9, 0.7)]
    kernel = 2 * Matern52Kernel(np.ones(2), ndim=2)
    models.append(GaussianProcessMCMC(kernel, prior=DefaultPrior(len(kernel) + 1, rng=np.random.RandomState(3)), n_hypers=8,
                                      chain_length=4, burnin_steps=2, rng=np.random.RandomState(4), lower=_BOX[0], upper=_BOX[1]))
    for o, m in enumerate(models):
        m.train(X, Y[:, min(o, 2)].copy(), **({"do_optimize": False} if o < 3 else {}))
    front, idx = pareto_front(Y, _REF3)
    for ms, native in ((models[:3], True), (models[:2] + models[3:], False)):
        acq = EHVI(ms, _REF3)
        assert acq._is_native() == native and np.allclose(acq.front, front, rtol=1e-14, atol=0) and len(front) >= 3
        a, mom = acq.compute(Xc), np.array(acq.moments(Xc))
        _within(a, mom[0::2], mom[1::2], acq.front, _REF3, "class native = %s" % native)
        assert acq.argmax(Xc) == EO.np_argmax(a) == acq.last_argmax and a.max() > 0
        x_inc, y_inc = acq.model.get_incumbent()
        j = idx[np.argmax(exclusive_contributions(front, _REF3))]
        assert np.allclose(x_inc, X[j], atol=1e-15) and np.allclose(y_inc, Y[j], rtol=1e-14)
    with pytest.raises(ValueError):
        EHVI(models + models[:1], np.full(5, 2.5))
    rng = np.random.RandomState(1)
    Yr = np.array([_toy3(rng.uniform(_BOX[0], _BOX[1])) for _ in range(8)])
    np.random.seed(1)
    res = multi_objective_optimization(_toy3, _BOX[0], _BOX[1], _REF3, num_iterations=8, n_init=3, n_candidates=128,
                                       rng=np.random.RandomState(1))
    Y, hv = np.array(res["Y"]), np.array(res["hypervolume"])
    front, idx = pareto_front(Y, _REF3)
    assert Y.shape == (8, 3) and np.all(np.diff(hv) >= 0) and hv[-1] == hypervolume(front, _REF3), hv
    assert hv[-1] >= hypervolume(pareto_front(Yr, _REF3)[0], _REF3)
    assert _bits(res["pareto_Y"], front) and _bits(res["pareto_X"], np.array(res["X"])[idx])


_CHECKS = [(_check_values, (K, P)) for K in (2, 3, 4) for P in (0, 1, 2, 7, 13)] + [(_check_values, (3, 64))] + \
    [(_check_k2, (P,)) for P in (0, NL - 2, NL - 1, NL)] + [(f, ()) for f in (_check_edges, _check_fused, _check_classes)]
_IDS = ["%s%s" % (f.__name__[7:], "-".join(map(str, a))) for f, a in _CHECKS]


@pytest.mark.parametrize("check,args", _CHECKS, ids=_IDS)
def test_emu(emu_ctx, check, args):
    check(emu_ctx, *args)


@pytest.mark.gpu
@pytest.mark.parametrize("check,args", _CHECKS, ids=_IDS)
def test_gpu(gpu_ctx, check, args):
    check(gpu_ctx, *args)


@pytest.mark.gpu
def test_fused_large_gpu(gpu_ctx):
    """N = 256, D = 4, K = 3, a front of 50 points, m = 32 773: every 97th candidate and the last six against the oracle"""
    M = 32768 + 5
    _check_fused(gpu_ctx, N=256, D=4, M=M, P=50, rows=np.concatenate((np.arange(0, M, 97), np.arange(M - 6, M))))
