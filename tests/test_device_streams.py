"""The random streams the device draws for itself, replayed counter for counter on the host (tests/streams_oracle.py on
bohamiann_oracle.philox), as include/robo_hip.h states them: robo_cand_create_uniform and robo_cand_create_random
(acq.hip) and the z = NULL draws of robo_acq_cmaes_cand (cmaes.hip).  The host Philox itself is held to the Random123
known answers, through an independent scalar restatement.

Uniforms are integer arithmetic and exact conversions: compared bit for bit.  A Box-Muller value is allowed the project's
bound for the device's evaluation, 16 eps rad (test_bohamiann.py's dxi), against the long-double replay; a Gaussian
candidate loc + scale g that bound scaled + 2 eps |loc + scale g| for the multiply-add, contracted or not, and the clip to
[0, 1] is 1-Lipschitz, so the bound holds after it and no element is exempted.  Largest error / bound observed: NOTES.md.
CPU: the interpreter; -m gpu: the MI355X.
"""
import os
import sys

import numpy as np
import pytest

from robo_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import streams_oracle as SO  # noqa: E402
from bohamiann_oracle import philox  # noqa: E402
from test_cmaes import _models, emu_ctx, gpu_ctx  # noqa: E402,F401

LD, EPS = SO.LD, SO.EPS
M32 = 0xFFFFFFFF
# 0: both key words zero; 123: k1 zero; both words live; the last differs from seed 0 through k1 alone
SEEDS = (0, 123, 0x1234567887654321, 0xFFFFFFFF00000000)
SHAPES = ((1, 1), (1, 2), (3, 1), (127, 3), (128, 3), (129, 3), (130, 5), (129, 64))
GRID = 8192 * 256                 # the threads of the largest launch: a block index from here on is a second trip of a thread

KNOWN_ANSWERS = (                 # Random123's kat_vectors for philox4x32_10: counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((M32, M32, M32, M32), (M32, M32), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def ctx(request):
    return request.getfixturevalue(request.param + "_ctx")


def _philox_words(counter, key):
    """Philox-4x32-10 on Python integers, from the paper: one block -> its four output words"""
    c, k = list(counter), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return tuple(c)


def _uniforms(w):
    return ((w[0] << 32 | w[1]) >> 11) * 2.0 ** -53, ((w[2] << 32 | w[3]) >> 11) * 2.0 ** -53


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_known_answers():
    """the published vectors: the scalar restatement gives the words, the array oracle the uniforms of exactly those words,
    and on other counters and keys (every word live, counters as arrays) the two agree with each other"""
    for counter, key, words in KNOWN_ANSWERS:
        assert _philox_words(counter, key) == words
        ua, ub = philox(*counter, key[0] | key[1] << 32)
        assert (float(ua), float(ub)) == _uniforms(words)
    rs = np.random.RandomState(0)
    cs, seed = rs.randint(0, 2 ** 32, size=(4, 64), dtype=np.uint64), 0x1234567887654321
    ua, ub = philox(*cs, seed)
    for j in range(cs.shape[1]):
        assert (ua[j], ub[j]) == _uniforms(_philox_words([int(c) for c in cs[:, j]], (seed & M32, seed >> 32)))


def test_shapes_reach_the_edges():
    """what SHAPES must cover.  m_pad is a multiple of 128, so m_pad dim is even for every shape: through this interface the
    last block always has both halves inside the array.  What can be reached is its neighbour: an array whose last real
    element is a block's second half (m = m_pad, the element a tail test that is off by one drops), and m dim odd, where
    the block (m dim - 1) / 2 straddles the last real row m - 1 and the first pad row m"""
    assert all(SO.padded(m) * dim % 2 == 0 for m, dim in SHAPES)
    assert any(SO.padded(m) == m for m, dim in SHAPES) and any(m * dim % 2 == 1 and SO.padded(m) > m for m, dim in SHAPES)
    assert any(m * dim > 2 * 256 for m, dim in SHAPES) and any(dim % 2 == 1 and m > 1 for m, dim in SHAPES)


@pytest.mark.parametrize("m,dim", SHAPES)
def test_uniform_candidates(ctx, m, dim):
    """robo_cand_create_uniform, bit for bit.  (Counter word 1, p >> 32, is live from 2^33 elements on: not reached.)"""
    got = {}
    for seed in SEEDS:
        cand = _lib.Candidates(ctx, m=m, dim=dim, seed=seed)
        got[seed] = cand.points()
        want = SO.uniform(philox, seed, m, dim)
        assert got[seed].shape == (m, dim) and _bits(got[seed], want), (m, dim, hex(seed))
        for i in {0, m // 2, m - 1}:
            assert _bits(cand.point(i), want[i])
        cand.close()
    assert np.all(got[SEEDS[3]] != got[SEEDS[0]])          # the high key word alone moves every element


def test_uniform_candidates_past_one_grid(ctx):
    """more blocks than the largest launch has threads: the second trip through the grid-stride loop"""
    m, dim, seed = 600_000, 7, SEEDS[2]
    assert SO.padded(m) * dim > 2 * GRID
    first = (2 * GRID) // dim                              # the first row that holds an element of a block >= GRID
    assert first < m - 1 and ((first + 1) * dim - 1) // 2 >= GRID
    cand = _lib.Candidates(ctx, m=m, dim=dim, seed=seed)
    want = SO.uniform(philox, seed, m, dim)
    assert _bits(cand.points(), want)
    for i in (0, first, first + 1, m - 1):
        assert _bits(cand.point(i), want[i]), i
    cand.close()


LOC = {1: [0.5], 2: [0.02, 0.99], 3: [0.02, 0.99, 0.5], 5: [0.02, 0.99, 0.5, 0.3, 0.7]}
SCALE = {1: [0.5], 2: [0.1, 0.05], 3: [0.1, 0.05, 0.02], 5: [0.1, 0.05, 0.02, 0.25, 0.3]}
N_UNIFORM = (0, 1, 64, 91, 129, 130)


def _check_random(ctx, seed, m, n_uniform, loc, scale):
    """one handle against the replay of its stream -> the largest error / bound of its Gaussian elements"""
    dim = len(loc)
    want = SO.random_sampling(philox, seed, m, dim, n_uniform, loc, scale)
    flat, gauss = want["branch"].ravel(), want["branch"] > 0
    assert np.all(flat[:n_uniform * dim] == 0) and np.all(flat[n_uniform * dim:] == 1 + np.arange(n_uniform * dim, m * dim) % 2)
    if dim % 2 == 1 and n_uniform % 2 == 1 and n_uniform < m:
        # the block across the rows n_uniform - 1 | n_uniform: a plain uniform, then a sine branch
        assert tuple(flat[n_uniform * dim - 1:n_uniform * dim + 1]) == (0, 2) and (n_uniform * dim - 1) % 2 == 0
    if gauss.sum() >= 39 * dim:                            # both clips occur, from the oracle alone
        assert np.any(want["raw"][gauss] < 0) and np.any(want["raw"][gauss] > 1)
        assert np.any(want["point"][gauss] == 0) and np.any(want["point"][gauss] == 1)
    cand = _lib.Candidates(ctx, m=m, seed=seed, n_uniform=n_uniform, loc=np.array(loc), scale=np.array(scale))
    got = cand.points()
    assert got.shape == (m, dim) and _bits(got[~gauss], want["point"][~gauss]), (hex(seed), dim, n_uniform)
    err = np.abs(got.astype(LD) - want["point"])[gauss]
    bound = want["bound"][gauss]
    assert np.all(bound > 0) and np.all(err <= bound), (hex(seed), dim, n_uniform, float((err / bound).max()))
    assert np.all((got >= 0) & (got <= 1))
    for i in {0, max(n_uniform - 1, 0), min(n_uniform, m - 1), m - 1}:
        assert _bits(cand.point(i), got[i])
    cand.close()
    return float((err / bound).max(initial=0.0))


def test_random_cases_reach_the_edges():
    cases = [(d, nu) for d in LOC for nu in N_UNIFORM]
    assert any(d % 2 == 1 and nu % 2 == 1 and 0 < nu < 130 and d > 1 for d, nu in cases)
    for d in LOC:
        assert len(LOC[d]) == len(SCALE[d]) == d
    for d in (3, 5):
        assert 0.02 in LOC[d] and 0.99 in LOC[d] and any(0.3 <= a <= 0.7 and s == 0.02 for a, s in zip(LOC[d], SCALE[d]))


@pytest.mark.parametrize("n_uniform", N_UNIFORM)
@pytest.mark.parametrize("dim", sorted(LOC))
def test_random_candidates(ctx, dim, n_uniform):
    """robo_cand_create_random: rows < n_uniform bit for bit, the rest within the Box-Muller bound"""
    worst = max(_check_random(ctx, seed, 130, n_uniform, LOC[dim], SCALE[dim]) for seed in SEEDS)
    print("random candidates dim %d n_uniform %d: error / bound %.3f" % (dim, n_uniform, worst))


def test_random_candidates_sharded(ctx):
    """the shards DeviceRandomSampling forms (maximizers/random_sampling.py): rank r draws rows [b, e) of the recipe from
    its own stream seed + 7919 r, the uniform / Gaussian split kept globally"""
    n_samples, world, base, dim = 513, 3, SEEDS[2], 3
    nu, seen, worst = int(n_samples * .7), [], 0.0
    for r in range(world):
        b, e = _lib.shard_range(n_samples, r, world)
        seen.append(min(max(nu - b, 0), e - b))
        worst = max(worst, _check_random(ctx, base + 7919 * r, e - b, seen[-1], LOC[dim], SCALE[dim]))
    assert sum(seen) == nu and 0 < seen[-1] < e - b        # the split falls inside the last shard
    print("sharded random candidates: error / bound %.3f" % worst)


@pytest.mark.parametrize("D,L", [(2, 6), (2, 9), (5, 6), (5, 9)])
def test_cmaes_draws(ctx, D, L):
    """z = NULL: every draw of the trace is the Box-Muller branch of its block (generation, instance, sample, pair) --
    cosine at coordinate 2 pair, sine at 2 pair + 1, none for the last pair of an odd D --; the same run on the caller's z,
    fed the traced draws, is the z = NULL run bit for bit"""
    R, T, seed = 3, 4, SEEDS[2]
    rs, _, (gp,), y = _models(ctx, 40, D)
    cand = _lib.Candidates(ctx, rs.rand(40, D))
    try:
        own = gp.cmaes("log_ei", 0.0, y.min(), cand, R, L, T, 0.3, z=None, seed=seed, diagnostics=True)
        z, code = own.trace["z"], own.trace["code"]
        assert z.shape == (T + 1, R, L, D) and not z[0].any()
        live = code[1:] < 6                                # 6: stopped earlier, 7: unused -- their sample columns are zero
        assert live.sum() == R * T                         # sigma0 0.3 over four generations stops nothing
        worst = 0.0
        for g in range(T):
            for r in np.flatnonzero(live[g]):
                want, rad = SO.cmaes_normals(philox, seed, g, r, L, D)
                err, bound = np.abs(z[g + 1, r].astype(LD) - want), 16 * EPS * rad
                assert np.all(err <= bound), (g, r, float((err / bound).max()))
                worst = max(worst, float((err / bound).max()))
        print("cmaes draws D %d lambda %d: error / bound %.3f" % (D, L, worst))
        fed = gp.cmaes("log_ei", 0.0, y.min(), cand, R, L, T, 0.3, z=np.ascontiguousarray(z[1:]), diagnostics=True)
        assert set(fed.trace) == set(own.trace) and all(fed.trace[k].tobytes() == own.trace[k].tobytes() for k in own.trace)
        assert (fed.value, fed.instance, fed.flags, fed.x.tobytes()) == (own.value, own.instance, own.flags, own.x.tobytes())
        other = gp.cmaes("log_ei", 0.0, y.min(), cand, R, L, T, 0.3, z=None, seed=SEEDS[3], diagnostics=True).trace["z"]
        assert not np.any(other[1:] == z[1:])
    finally:
        cand.close()
        gp.close()
