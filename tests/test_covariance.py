"""The covariance paths on a real MI355X against the extended-precision oracle (tests/cov_checks.py).  ``pytest -m gpu``."""
import os

import pytest

import cov_checks as C
from robo_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    _lib.use_library(None)
    assert os.path.exists(_lib.DEFAULT_LIBRARY), "librobo_hip.so missing: the GPU tests never fall back"
    c = _lib.Context(0)
    assert "hipemu" not in c.name
    yield c
    c.close()


@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("kind", ["matern52", "rbf", "fabolas"])
def test_scalar_range_sweep(ctx, kind, fp32):
    """C1: pos_sqrt / exp_nonpos (fp64) and the library's sqrtf / expf (fp32) from r2 = 1e-300 to 1e300, through the gram
    tiles, the cross-gram kernel and cov_rows"""
    C.check_scalar_sweep(ctx, kind, fp32)


@pytest.mark.parametrize("D", [1, 15, 16, 17, 33])
def test_distance_geometry(ctx, D):
    """C2: K entry by entry over N in {63, 64, 126, 130, 200} x ln m in {-10, -4, 0, 2, mixed}, near and exact duplicates"""
    C.check_geometry(ctx, [c for c in C.geometry_cases() if c[0] == D or (D == 15 and c[0] == 3)])


@pytest.mark.parametrize("N,D", C.FEED_CASES)
def test_what_the_entries_feed(ctx, N, D):
    """C3: likelihoods, chain log-probabilities, gradient and posterior at the prior's short end with near-duplicate rows"""
    C.check_feeds(ctx, N, D)


@pytest.mark.parametrize("fp32,d_in", C.FABOLAS_CASES)
def test_fabolas_products(ctx, fp32, d_in):
    """C4: the split product / exponent form stays finite where the bare product overflows"""
    C.check_fabolas_products(ctx, fp32, d_in)
