"""What the ensemble entry points refuse, and how (tests/ensemble_checks.py): robo_acq_refine_*, robo_acq_batch_* and
robo_mes_eval_* share one validation of (models, S, incumbents, candidates); this file pins the verdict of every family
and form so that the shared code cannot change one of them unnoticed.

CPU: through the interpreter (tests/hipemu).  -m gpu: the same rows through the real library on the MI355X.
"""
import os
import sys

import pytest

import ensemble_checks as E
from robo_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu_ctx():
    sys.path.insert(0, os.path.join(HERE, "hipemu"))
    import build_emu
    _lib.use_library(build_emu.build())
    ctx = _lib.Context(0)
    assert "hipemu" in ctx.name
    yield ctx
    ctx.close()
    _lib.use_library(None)


@pytest.fixture(scope="module")
def gpu_ctx():
    _lib.use_library(None)
    assert os.path.exists(_lib.DEFAULT_LIBRARY), "librobo_hip.so missing: the GPU tests never fall back"
    c = _lib.Context(0)
    assert "hipemu" not in c.name
    yield c
    c.close()


@pytest.mark.parametrize("family", E.FAMILIES)
def test_error_contract_emu(emu_ctx, family):
    E.check_family(emu_ctx, family)


@pytest.mark.gpu
@pytest.mark.parametrize("family", E.FAMILIES)
def test_error_contract_gpu(gpu_ctx, family):
    E.check_family(gpu_ctx, family)
