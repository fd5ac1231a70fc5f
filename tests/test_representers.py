"""Entropy search's representer points sampled on the device (robo_amd/csrc/represent.hip, robo_rep_sample /
robo_rep_sample_batch, InformationGain(representers="device"), MarginalizationGPMCMC's batched update) against the fp64
oracle through tests/rep_oracle.py and against the host sampler (robo_amd/util/ensemble_sampler.py).

Whole trajectories are not compared to the oracle: a rounding-level difference may flip one accept test and send two
correct chains apart.  Every step of the device's trace is checked on its own -- the proposal against NumPy's
c - z (c - s) bit for bit, the box verdict, the log-density against the oracle at the device's own q, the accept bit
against the rule applied to the device's own stored doubles -- and the final state against the replay of the trace.
Against the HOST sampler on the same library the whole chain is compared bit for bit.
CPU: through the interpreter (tests/hipemu), N = 40.  -m gpu: the MI355X at N = 300 (three 128-blocks, the last ragged),
k = 50 (25 movers), T = 50, S = 3, and at N = 129, D = 1, k = 2, T = 4.
"""
import os
import sys

import numpy as np
import pytest

from robo_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rep_oracle as RO  # noqa: E402
from _tol import ACQ_RTOL, assert_logei_close  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402

EMU1 = dict(name="emu1", N=40, D=1, k=8, T=6, S=1)
EMU3 = dict(name="emu3", N=40, D=3, k=8, T=6, S=3)
LARGE = dict(name="large", N=300, D=3, k=50, T=50, S=3)
TINY = dict(name="tiny", N=129, D=1, k=2, T=4, S=1)
BOX_LO, BOX_HI = np.array([-1.0, 0.5, 2.0]), np.array([3.0, 1.5, 2.5])
# Seeds per (case, kind, normalised inputs), chosen on the CPU oracle alone (test_seeds_hold_on_the_oracle keeps them
# honest): the lowest seed whose oracle chains contain a rejected, an accepted and an out-of-box proposal and no accept
# decision closer than NEAR (relative) to its threshold.
NEAR = 1e-6
SEEDS = {
    ("emu1", "ei", False): 1,
    ("emu1", "ei", True): 1,
    ("emu1", "log_ei", False): 0,
    ("emu1", "log_ei", True): 0,
    ("emu1", "pi", False): 0,
    ("emu1", "pi", True): 0,
    ("emu1", "lcb", False): 0,
    ("emu1", "lcb", True): 0,
    ("emu3", "ei", False): 0,
    ("emu3", "ei", True): 0,
    ("emu3", "log_ei", False): 0,
    ("emu3", "log_ei", True): 0,
    ("emu3", "pi", False): 0,
    ("emu3", "pi", True): 0,
    ("emu3", "lcb", False): 0,
    ("emu3", "lcb", True): 0,
    ("large", "ei", False): 0,
    ("large", "ei", True): 0,
    ("large", "log_ei", False): 0,
    ("large", "log_ei", True): 0,
    ("large", "pi", False): 0,
    ("large", "pi", True): 0,
    ("large", "lcb", False): 0,
    ("large", "lcb", True): 0,
    ("tiny", "log_ei", False): 1,
    ("tiny", "log_ei", True): 1,
    ("tiny", "lcb", False): 1,
    ("tiny", "lcb", True): 1,
    ("tiny", "ei", False): 1,
    ("tiny", "ei", True): 1,
    ("tiny", "pi", False): 1,
    ("tiny", "pi", True): 1,
}


@pytest.fixture(scope="module")
def emu_ctx():
    sys.path.insert(0, os.path.join(HERE, "hipemu"))
    import build_emu
    _lib.use_library(build_emu.build())
    ctx = _lib.default_context()
    assert "hipemu" in ctx.name
    yield ctx
    _lib.use_library(None)


@pytest.fixture(scope="module")
def gpu_ctx():
    _lib.use_library(None)
    if _lib.device_count() < 1:
        pytest.skip("no HIP device")
    yield _lib.default_context()


# ---- helpers ---------------------------------------------------------------------------------------------------------
def _theta(D, ls2, noise):
    return np.concatenate([[0.0], np.log(np.broadcast_to(ls2, (D,))), [np.log(noise)]])


def _problem(case, normalize, seed):
    """S oracle GPs (different thetas and incumbents) on one data set, start positions with every other walker within
    0.02 of a box face, and the draws of T ensemble steps per chain"""
    N, D, k, T, S = (case[x] for x in ("N", "D", "k", "T", "S"))
    rs = np.random.RandomState(seed)
    lo, hi = (BOX_LO[:D], BOX_HI[:D]) if normalize else (np.zeros(D), np.ones(D))
    U = rs.rand(N, D)
    X = lo + (hi - lo) * U
    y = np.sin(3 * U.sum(axis=1) / np.sqrt(D / 3.0)) + 0.1 * rs.randn(N)
    ogps, thetas = [], []
    for s in range(S):
        theta = _theta(D, np.array([0.3, 0.5, 0.8])[:D] * (1.0 + 0.3 * s), 1e-2 * (1 + s))
        ogp = O.OracleGP("matern52", theta, normalize_input=normalize, lower=lo, upper=hi)
        ogp.train(X, y)
        ogps.append(ogp)
        thetas.append(theta)
    # incumbents at the targets' median: EI and PI, taken as log-densities as they stand, then vary by O(1) over the box
    # (at the observed minimum both are ~0 everywhere on dense data and no proposal inside the box is ever rejected)
    etas = np.array([np.median(y) + 0.05 * s for s in range(S)])
    half = k // 2
    p0 = lo + (hi - lo) * rs.rand(S, k, D)
    near = 0.02 * rs.rand(S, k) * (hi[0] - lo[0])
    p0[:, 1::4, 0] = (lo[0] + near)[:, 1::4]
    p0[:, 3::4, 0] = (hi[0] - near)[:, 3::4]
    uz, ua = rs.rand(S, T, 2, half), rs.rand(S, T, 2, half)
    pa = rs.randint(half, size=(S, T, 2, half)).astype(np.int32)
    return dict(case=case, normalize=normalize, lo=lo, hi=hi, ogps=ogps, thetas=thetas, etas=etas, p0=p0, uz=uz, pa=pa, ua=ua)


def _oracle_chains(prob, kind, par):
    return [RO.chain(RO.lnprob(prob["ogps"][s], kind, par, prob["etas"][s], prob["lo"], prob["hi"]), prob["lo"], prob["hi"],
                     prob["p0"][s], prob["uz"][s], prob["pa"][s], prob["ua"][s]) for s in range(prob["case"]["S"])]


def _seed_ok(case, kind, par, normalize, seed):
    runs = _oracle_chains(_problem(case, normalize, seed), kind, par)
    codes = np.concatenate([r["codes"].ravel() for r in runs])
    margin = min(r["margin"].min() for r in runs)
    return set(codes) == {0, 1, 2} and margin > NEAR and all(np.all(np.isfinite(r["lnp"])) for r in runs)


def _device_gps(ctx, prob):
    gps = []
    for ogp, theta in zip(prob["ogps"], prob["thetas"]):
        g = _lib.DeviceGP(ctx, "matern52", ogp.X.shape[0], ogp.X.shape[1])
        g.set_data(ogp.X, ogp.y)
        g.fit(theta, ogp.mean)
        gps.append(g)
    return gps


def _run(gps, prob, kind, par, lnp=None, T=None, diagnostics=True, chains=None):
    """rep_sample_batch over the problem's chains (``chains``: a selection, in the order given)"""
    idx = list(range(len(gps))) if chains is None else list(chains)
    T = prob["case"]["T"] if T is None else T
    return _lib.rep_sample_batch([gps[i] for i in idx], kind, par, prob["etas"][idx], prob["lo"], prob["hi"],
                                 prob["normalize"], prob["p0"][idx], None if lnp is None else lnp[idx], T,
                                 prob["uz"][idx, :T], prob["pa"][idx, :T], prob["ua"][idx, :T], diagnostics=diagnostics)


def _check_chain(prob, s, kind, par, lnp0, pos, lnp, acc, trace, tally):
    """one chain's trace, step by step, on the device's own doubles; final state = the replay"""
    lo, hi, D = prob["lo"], prob["hi"], prob["case"]["D"]
    k, half = prob["case"]["k"], prob["case"]["k"] // 2
    uz, pa, ua = prob["uz"][s], prob["pa"][s], prob["ua"][s]
    p, lp, n = prob["p0"][s].copy(), lnp0.copy(), np.zeros(k, dtype=np.int64)
    Q, F = [], []
    for it in range(trace.shape[0]):
        for h in range(2):
            S0, S1 = slice(h * half, (h + 1) * half), slice((1 - h) * half, (2 - h) * half)
            z, q = RO.stretch(p[S1][pa[it, h]], p[S0], uz[it, h])
            np.testing.assert_array_equal(trace[it, h, :, :D], q)                 # NumPy's c - z (c - s), bit for bit
            out = RO.outside(q, lo, hi)
            lq, code = trace[it, h, :, D], trace[it, h, :, D + 1]
            np.testing.assert_array_equal(code == 2, out)
            assert np.all(np.isin(code, (0, 1, 2))) and np.all(np.isneginf(lq[out])) and not np.any(np.isnan(lq))
            Q.append(q[~out])
            F.append(lq[~out])
            with np.errstate(invalid="ignore"):
                diff = (D - 1.0) * np.log(z) + lq - lp[S0]
            lu = np.log(ua[it, h])
            want, got = diff > lu, code == 1
            for w in np.nonzero(want != got)[0]:
                big = max(abs(diff[w]), abs(lu[w]))
                assert np.isfinite(diff[w]) and abs(diff[w] - lu[w]) <= 64 * np.spacing(big), (it, h, w, diff[w], lu[w])
                tally["excused"] += 1
            tally["decisions"] += half
            idx = np.arange(k)[S0][got]
            p[idx], lp[idx] = q[got], lq[got]
            n[idx] += 1
            tally["codes"].update(int(c) for c in code)
    np.testing.assert_array_equal(pos, p)
    np.testing.assert_array_equal(lnp, lp)
    np.testing.assert_array_equal(acc, n)
    # the log-density against the oracle at the device's own points (start positions included)
    ogp, eta = prob["ogps"][s], prob["etas"][s]
    P = np.concatenate([prob["p0"][s][~RO.outside(prob["p0"][s], lo, hi)]] + Q)
    fd = np.concatenate([lnp0[~RO.outside(prob["p0"][s], lo, hi)]] + F)
    fo = RO.lnprob(ogp, kind, par, eta, lo, hi)(P)
    with np.errstate(divide="ignore", invalid="ignore"):
        print("%s chain %d %s: %d values, max rel error %.3e" % (prob["case"]["name"], s, kind, P.shape[0],
                                                                 np.nanmax(np.abs(fd - fo) / np.abs(fo))))
    if kind == "log_ei":
        assert_logei_close(fd, fo, RO.z_of(ogp, par, eta, P), rtol=ACQ_RTOL, tail_rtol=ACQ_RTOL)
    else:
        np.testing.assert_allclose(fd, fo, rtol=ACQ_RTOL, atol=0)


def check_steps(ctx, case, kind, par, normalize):
    """check 1: every step of every chain on its own"""
    prob = _problem(case, normalize, SEEDS[(case["name"], kind, normalize)])
    gps = _device_gps(ctx, prob)
    try:
        _, lnp0, acc0, flags0, _ = _run(gps, prob, kind, par, T=0)
        assert not np.any(acc0) and not np.any(flags0)
        pos, lnp, acc, flags, trace = _run(gps, prob, kind, par, lnp=lnp0)
        assert not np.any(flags)
        tally = dict(excused=0, decisions=0, codes=set())
        for s in range(case["S"]):
            _check_chain(prob, s, kind, par, lnp0[s], pos[s], lnp[s], acc[s], trace[s], tally)
        assert tally["codes"] == {0, 1, 2}, tally
        assert 100 * tally["excused"] <= tally["decisions"], tally
    finally:
        for g in gps:
            g.close()


def check_batch_equals_single(ctx, case):
    """check 3: chain s of the batch == robo_rep_sample on gps[s]; S and the chain's index change nothing"""
    kind, par = "log_ei", 0.0
    prob = _problem(case, True, SEEDS[(case["name"], kind, True)])
    gps = _device_gps(ctx, prob)
    try:
        batch = _run(gps, prob, kind, par)
        S = case["S"]
        for s in range(S):
            one = _lib.rep_sample(gps[s], kind, par, prob["etas"][s], prob["lo"], prob["hi"], True, prob["p0"][s], None,
                                  case["T"], prob["uz"][s], prob["pa"][s], prob["ua"][s], diagnostics=True)
            for a, b in zip(one, batch):
                np.testing.assert_array_equal(a, b[s])
        if S > 1:
            order = list(range(S))[::-1][:S - 1]             # fewer chains, other slots
            part = _run(gps, prob, kind, par, chains=order)
            for j, s in enumerate(order):
                for a, b in zip(part, batch):
                    np.testing.assert_array_equal(a[j], b[s])
    finally:
        for g in gps:
            g.close()


def check_shape_change(ctx):
    """one live handle through the state-block shapes (4 walkers, 3 steps) -> (8 walkers, 2 steps) -> the first again: the
    block grows once, and every call gives the bits of a handle that never held another shape (N = 22, D = 2: every
    array of the block is non-empty and odd counts make the 16-byte round-up between the arrays matter)"""
    kind, par = "log_ei", 0.0
    small = _problem(dict(name="small", N=22, D=2, k=4, T=3, S=1), True, 0)
    large = _problem(dict(name="large", N=22, D=2, k=8, T=2, S=1), True, 0)
    assert np.array_equal(small["ogps"][0].X, large["ogps"][0].X)          # one model: the data are the seed's first draws
    live, fresh = gps = _device_gps(ctx, small) + _device_gps(ctx, large)
    try:
        first, more, again = _run([live], small, kind, par), _run([live], large, kind, par), _run([live], small, kind, par)
        for a, b in zip(first + more, again + _run([fresh], large, kind, par)):
            assert a.tobytes() == b.tobytes()
    finally:
        for g in gps:
            g.close()


def _model(N, D, seed, ls2=0.3, noise=1e-3):
    """a trained robo_amd GaussianProcess on the library in use, inputs normalised from BOX"""
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models.gaussian_process import GaussianProcess
    rs = np.random.RandomState(seed)
    lo, hi = BOX_LO[:D], BOX_HI[:D]
    U = rs.rand(N, D)
    y = np.sin(3 * U.sum(axis=1) / np.sqrt(D / 3.0)) + 0.1 * rs.randn(N)
    model = GaussianProcess(2 * Matern52Kernel(np.full(D, ls2), ndim=D), noise=noise, lower=lo, upper=hi,
                            rng=np.random.RandomState(3))
    model.train(lo + (hi - lo) * U, y, do_optimize=False)
    return model, lo, hi


def _start(lo, hi, k, seed):
    rs = np.random.RandomState(seed)
    p0 = lo + (hi - lo) * rs.rand(k, lo.shape[0])
    p0[1::2, 0] = lo[0] + 0.02 * rs.rand(k // 2) * (hi[0] - lo[0])
    return p0


def _sampler_runs(ig, p0, T, seed, chains):
    from robo_amd.util.ensemble_sampler import EnsembleSampler
    out = []
    for dc in chains:
        s = EnsembleSampler(p0.shape[0], p0.shape[1], lnprob_batch=ig._proposal_batch, device_chain=dc)
        s._random = np.random.RandomState(seed)
        p, lp, state = s.run_mcmc(p0, T)
        out.append((p, lp, s.chain, s.lnprobability, s.naccepted, state[1], np.array(state[2])))
    return out


def check_equals_host_sampler(case, sampling):
    """check 2: the host loop around _proposal_batch and the device chain, same library, same stream: identical bits"""
    from robo_amd.acquisition_functions import EI, InformationGain
    N, D, k, T = (case[x] for x in ("N", "D", "k", "T"))
    model, lo, hi = _model(N, D, 1)
    ig = InformationGain(model, lo, hi, Nb=k, sampling_acquisition=EI if sampling == "ei" else None,
                         representers="device")
    ig.sampling_acquisition.update(model)
    host, dev = _sampler_runs(ig, _start(lo, hi, k, 2), T, 11, (None, ig._device_chain()))
    for a, b in zip(host, dev):
        np.testing.assert_array_equal(a, b)
    assert 0 < host[4].sum() < k * T                         # moves were accepted and rejected
    model.gp.close()


def check_protocol(ctx, case):
    """check 4"""
    kind, par = "log_ei", 0.0
    prob = _problem(case, True, SEEDS[(case["name"], kind, True)])
    gps = _device_gps(ctx, prob)
    k, D, T = case["k"], case["D"], case["T"]
    g, eta, lo, hi = gps[0], prob["etas"][0], prob["lo"], prob["hi"]
    p0, uz, pa, ua = prob["p0"][0], prob["uz"][0], prob["pa"][0], prob["ua"][0]
    half = k // 2

    def single(gp=g, lower=lo, upper=hi, pos=p0, lnp=None, steps=T, draws=(uz, pa, ua), kind=kind, eta=eta, trace=False):
        return _lib.rep_sample(gp, kind, par, eta, lower, upper, True, pos, lnp, steps, draws[0][:steps], draws[1][:steps],
                               draws[2][:steps], diagnostics=trace)
    try:
        # argument errors: status and message
        with pytest.raises(ValueError, match="must be even"):
            single(pos=np.vstack([p0, p0[:1]]), draws=(uz, pa, ua), steps=0)
        if D > 1:
            with pytest.raises(ValueError, match="at least twice the dimension"):
                single(pos=p0[:2 * D - 2], steps=0)
        bad_hi = hi.copy()
        bad_hi[0] = lo[0]
        with pytest.raises(ValueError, match="is not below upper"):
            single(upper=bad_hi)
        with pytest.raises(ValueError, match="partner index"):
            single(draws=(uz, pa + half, ua))
        fresh = _lib.DeviceGP(ctx, "matern52", case["N"], D)
        with pytest.raises(Exception, match="Model has to be trained first!"):
            single(gp=fresh)
        fresh.close()
        two = np.array([p0, p0])
        draws2 = [np.array([d, d]) for d in (uz, pa, ua)]

        def pair(a, b):
            return _lib.rep_sample_batch([a, b], kind, par, [eta, eta], lo, hi, True, two, None, T, *draws2)
        other = _lib.Context(0)
        og = _lib.DeviceGP(other, "matern52", case["N"], D)
        og.set_data(prob["ogps"][0].X, prob["ogps"][0].y)
        og.fit(prob["thetas"][0], prob["ogps"][0].mean)
        with pytest.raises(_lib.RoboBadShape, match="context"):
            pair(g, og)
        og.close()
        other.close()
        small = _lib.DeviceGP(ctx, "matern52", case["N"] - 3, D)
        small.set_data(prob["ogps"][0].X[:-3], prob["ogps"][0].y[:-3])
        small.fit(prob["thetas"][0], prob["ogps"][0].mean)
        with pytest.raises(_lib.RoboBadShape, match="does not match"):
            pair(g, small)
        small.close()
        wide = _lib.DeviceGP(ctx, "matern52", case["N"], D + 1)
        wide.set_data(np.hstack([prob["ogps"][0].X, prob["ogps"][0].X[:, :1]]), prob["ogps"][0].y)
        wide.fit(_theta(D + 1, 0.5, 1e-2), prob["ogps"][0].mean)
        with pytest.raises(_lib.RoboBadShape, match="does not match"):
            pair(g, wide)
        wide.close()
        with pytest.raises(ValueError, match="share a model handle"):
            pair(g, g)
        # lnp0 given == evaluated; T = 0 is the start evaluation
        start = single(steps=0)
        np.testing.assert_array_equal(start[0], p0)
        fo = RO.lnprob(prob["ogps"][0], kind, par, eta, lo, hi)(p0)
        assert_logei_close(start[1], fo, RO.z_of(prob["ogps"][0], par, eta, p0), rtol=ACQ_RTOL, tail_rtol=ACQ_RTOL)
        assert not np.any(start[2]) and start[3] == 0
        a, b = single(trace=True), single(lnp=start[1], trace=True)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
        # every walker outside the box: all -inf, nothing moves, no NaN
        gone = single(pos=hi + (hi - lo) * (1.0 + p0 - lo), trace=True)
        assert np.all(np.isneginf(gone[1])) and not np.any(gone[2]) and gone[3] == 0
        assert np.all(gone[4][..., D + 1] != 1) and not np.any(np.isnan(gone[4]))
        # the flag word is per chain: a NaN incumbent in chain 1 leaves chain 0 clean
        res = _lib.rep_sample_batch(gps[:2], "ei", par, [eta, np.nan], lo, hi, True, two, None, 1,
                                    *[d[:, :1] for d in draws2])
        assert res[3][0] == 0 and res[3][1] & _lib.FLAG_NAN
        # rows that do not fit the solve workspace: ROBO_BAD_SHAPE
        try:
            ctx.set_tuning("ws_bytes", 1024)
            with pytest.raises(_lib.RoboBadShape, match="solve workspace"):
                single()
        finally:
            ctx.set_tuning("ws_bytes", None)
    finally:
        for x in gps:
            x.close()


def check_declined_call_falls_back(ctx, case):
    """check 4, last item: the library declines (workspace) -> the host loop with the same draws == representers="host" """
    from robo_amd.acquisition_functions import InformationGain
    model, lo, hi = _model(case["N"], case["D"], 1)
    k, T = case["k"], case["T"]
    ig = InformationGain(model, lo, hi, Nb=k, representers="device")
    ig.sampling_acquisition.update(model)
    p0 = _start(lo, hi, k, 2)
    host = _sampler_runs(ig, p0, T, 11, (None,))[0]
    try:
        ctx.set_tuning("ws_bytes", 1024)
        declined = _sampler_runs(ig, p0, T, 11, (ig._device_chain(),))[0]
    finally:
        ctx.set_tuning("ws_bytes", None)
    for a, b in zip(host, declined):
        np.testing.assert_array_equal(a, b)
    model.gp.close()


def _seeded_streams(monkeypatch, seed=5):
    from robo_amd.acquisition_functions.information_gain import InformationGain
    monkeypatch.setattr(InformationGain, "_sampler_stream", staticmethod(lambda: np.random.RandomState(seed)))


def check_information_gain_update(case, monkeypatch, mc=False):
    """check 5: update() with representers="device" == "host" under a seeded sampler stream"""
    from robo_amd.acquisition_functions import InformationGain, InformationGainMC
    _seeded_streams(monkeypatch)
    model, lo, hi = _model(case["N"], case["D"], 1)
    states = []
    for rep in ("host", "device"):
        if mc:
            ig = InformationGainMC(model, lo, hi, Nb=case["k"], Np=8, Nf=50, rng=np.random.RandomState(1), representers=rep)
        else:
            ig = InformationGain(model, lo, hi, Nb=case["k"], Np=20, rng=np.random.RandomState(1), representers=rep)
        ig.sampler_steps = case["T"]
        ig.update(model)
        states.append((ig.zb, ig.lmb, ig.logP))
    for a, b in zip(*states):
        np.testing.assert_array_equal(a, b)
    assert np.all(np.isfinite(states[0][1]))
    model.gp.close()


class _Samples(object):
    """stands in for a GaussianProcessMCMC: MarginalizationGPMCMC reads ``models``"""

    def __init__(self, models):
        self.models = models


def check_marginal_update(case, monkeypatch, ep):
    """check 5: MarginalizationGPMCMC.update over S = 3 == estimator by estimator, one rep_sample_batch per context"""
    from robo_amd.acquisition_functions import InformationGain, MarginalizationGPMCMC
    _seeded_streams(monkeypatch)
    subs = [_model(case["N"], case["D"], 1, ls2=0.3 * (1 + s), noise=1e-3 * (1 + s))[0] for s in range(3)]
    lo, hi = BOX_LO[:case["D"]], BOX_HI[:case["D"]]
    model = _Samples(subs)
    calls = []
    real = _lib.rep_sample_batch
    monkeypatch.setattr(_lib, "rep_sample_batch", lambda *a, **kw: (calls.append(len(a[0])), real(*a, **kw))[1])
    states = []
    for batched in (True, False):
        base = InformationGain(subs[0], lo, hi, Nb=case["k"], Np=20, rng=np.random.RandomState(1), ep=ep,
                               representers="device")
        base.sampler_steps = case["T"]
        marg = MarginalizationGPMCMC.__new__(MarginalizationGPMCMC)
        marg.acquisition_func, marg.model, marg.cost_model, marg.estimators = base, model, None, []
        marg.last_max = marg.last_argmax = None
        marg.sample_shard = False
        marg._build_estimators()
        if not batched:
            monkeypatch.setattr(MarginalizationGPMCMC, "_update_representers_batched", lambda self: False)
        del calls[:]
        marg.update(model)
        if batched:
            assert calls == [3], calls                       # one context: exactly one call, all three chains in it
        states.append([(e.zb, e.lmb, e.logP, e.dlogPdMu, e.dlogPdSigma) for e in marg.estimators])
        vals = marg.compute(lo + (hi - lo) * np.random.RandomState(4).rand(5, case["D"]))
        assert vals.shape == (5,) and np.all(np.isfinite(vals))
    for ea, eb in zip(*states):
        for a, b in zip(ea, eb):
            np.testing.assert_array_equal(a, b)
    assert not np.array_equal(states[0][0][0], states[0][1][0])     # the samples' chains differ
    for m in subs:
        m.gp.close()


def check_front_end(model):
    from robo_amd.fmin import entropy_search
    r = entropy_search(lambda x: float((x[0] - 0.3) ** 2), np.zeros(1), np.ones(1), num_iterations=3, n_init=1, model=model,
                       rng=np.random.RandomState(0), n_candidates=10, n_representer=6, n_outcomes=8, chain_length=2,
                       burnin_steps=2, ep="device", representers="device")
    assert len(r["X"]) == 3 and np.isfinite(r["f_opt"]) and np.all(np.isfinite(r["x_opt"]))
    assert np.all(np.isfinite(r["incumbent_values"]))


# ---- without a GPU ---------------------------------------------------------------------------------------------------------
# Two tests only, on purpose: tests/conftest.py runs the files on worker processes in the order of their test counts, and a
# file that sorts in the middle reshuffles which files share a worker.  With two tests this file sorts last and the
# others keep their places.  Every check prints its name, so a failure is found with -s.
def check_seeds_hold_on_the_oracle():
    """every fixed seed: the oracle's own chains have a rejected, an accepted and an out-of-box proposal, end finite, and
    hold no accept decision within NEAR of its threshold"""
    for case in (EMU1, EMU3, LARGE, TINY):
        for kind, par in RO.KINDS:
            for normalize in (False, True):
                assert _seed_ok(case, kind, par, normalize, SEEDS[(case["name"], kind, normalize)]), (case["name"], kind)


def check_invalid_values_raise():
    from robo_amd.acquisition_functions import InformationGain, InformationGainMC
    from robo_amd.fmin.entropy_search import build_entropy_search
    for bad in ("gpu", "Device", 1):
        with pytest.raises(ValueError, match="representers"):
            InformationGain(None, np.zeros(2), np.ones(2), representers=bad)
        with pytest.raises(ValueError, match="representers"):
            InformationGainMC(None, np.zeros(2), np.ones(2), representers=bad)
    with pytest.raises(ValueError, match="representers"):
        build_entropy_search(np.zeros(1), np.ones(1), model="gp", representers="gpu")
    assert InformationGain(None, np.zeros(2), np.ones(2))._representers() == "host"          # the default stays the host


def check_fabolas_models_raise():
    from robo_amd.acquisition_functions import InformationGain
    from robo_amd.kernels import Matern52Kernel
    from robo_amd.models.fabolas_gp import FabolasGP
    model = FabolasGP(Matern52Kernel(np.ones(2), ndim=2), basis_function=lambda x: x, lower=np.zeros(2), upper=np.ones(2))
    ig = InformationGain(model, np.zeros(2), np.ones(2), Nb=4, representers="device")
    with pytest.raises(NotImplementedError, match="Fabolas"):
        ig.sample_representer_points()


def test_host_side():
    check_seeds_hold_on_the_oracle()
    check_invalid_values_raise()
    check_fabolas_models_raise()


def test_through_the_interpreter(emu_ctx):
    """the checks of the MI355X tests below at N = 40, D in {1, 3}, k = 8, T = 6, S in {1, 3}"""
    def step(name, fn, *args):
        print("interpreter:", name, args[1:] if args and args[0] is emu_ctx else args)
        with pytest.MonkeyPatch.context() as mp:
            fn(*[mp if a is MonkeyPatch else a for a in args])
    MonkeyPatch = object()
    for case in (EMU1, EMU3):
        for kind, par in RO.KINDS:
            for normalize in (False, True):
                step("every step", check_steps, emu_ctx, case, kind, par, normalize)
        for sampling in ("log_ei", "ei"):
            step("equals host sampler", check_equals_host_sampler, case, sampling)
    step("batch equals single", check_batch_equals_single, emu_ctx, EMU3)
    step("shape change on a live handle", check_shape_change, emu_ctx)
    step("protocol", check_protocol, emu_ctx, EMU3)
    step("declined call falls back", check_declined_call_falls_back, emu_ctx, EMU3)
    for mc in (False, True):
        step("information gain update", check_information_gain_update, EMU3, MonkeyPatch, mc)
    for ep in ("host", "device"):
        step("marginal update", check_marginal_update, EMU3, MonkeyPatch, ep)
    for model in ("gp", "gp_mcmc"):
        step("front end", check_front_end, model)


# ---- on the MI355X --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("kind,par", RO.KINDS)
@pytest.mark.parametrize("case", [LARGE, TINY], ids=["N300", "N129"])
def test_gpu_every_step(gpu_ctx, case, kind, par, normalize):
    check_steps(gpu_ctx, case, kind, par, normalize)


@pytest.mark.gpu
@pytest.mark.parametrize("sampling", ["log_ei", "ei"])
@pytest.mark.parametrize("case", [LARGE, TINY], ids=["N300", "N129"])
def test_gpu_equals_host_sampler(gpu_ctx, case, sampling):
    check_equals_host_sampler(case, sampling)


@pytest.mark.gpu
def test_gpu_batch_equals_single(gpu_ctx):
    check_batch_equals_single(gpu_ctx, LARGE)
    check_shape_change(gpu_ctx)


@pytest.mark.gpu
def test_gpu_protocol(gpu_ctx):
    check_protocol(gpu_ctx, LARGE)


@pytest.mark.gpu
def test_gpu_declined_call_falls_back(gpu_ctx):
    check_declined_call_falls_back(gpu_ctx, LARGE)


@pytest.mark.gpu
@pytest.mark.parametrize("mc", [False, True], ids=["ep", "mc"])
def test_gpu_information_gain_update(gpu_ctx, monkeypatch, mc):
    check_information_gain_update(LARGE, monkeypatch, mc)


@pytest.mark.gpu
@pytest.mark.parametrize("ep", ["host", "device"])
def test_gpu_marginal_update(gpu_ctx, monkeypatch, ep):
    check_marginal_update(LARGE, monkeypatch, ep)


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["gp", "gp_mcmc"])
def test_gpu_front_end(gpu_ctx, model):
    check_front_end(model)
