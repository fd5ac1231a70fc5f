"""tests/cov_checks.py through the interpreted build of the HIP sources (tests/hipemu): the tiles' index arithmetic, the
choice between the dot and the direct-difference form, the Fabolas folding and the host plumbing of the diagnostics entry
points.  The interpreter's rsq is exact and its exp is the host's: the claim about the device arithmetic is
tests/test_covariance.py (-m gpu)."""
import os
import sys

import pytest

import cov_checks as C
from robo_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu_ctx():
    sys.path.insert(0, os.path.join(HERE, "hipemu"))
    import build_emu
    path = build_emu.build()
    _lib.use_library(path)
    ctx = _lib.Context(0)
    assert "hipemu" in ctx.name
    yield ctx
    ctx.close()
    _lib.use_library(None)


def test_scalar_range_sweep(emu_ctx):
    for kind in ("matern52", "rbf", "fabolas"):
        for fp32 in (False, True):
            C.check_scalar_sweep(emu_ctx, kind, fp32)


def test_distance_geometry(emu_ctx):
    C.check_geometry(emu_ctx, C.geometry_cases())


def test_what_the_entries_feed(emu_ctx):
    for N, D in C.FEED_CASES:
        C.check_feeds(emu_ctx, N, D)


def test_fabolas_products(emu_ctx):
    for fp32, d_in in C.FABOLAS_CASES:
        C.check_fabolas_products(emu_ctx, fp32, d_in)
