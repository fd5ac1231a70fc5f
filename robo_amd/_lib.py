"""ctypes binding of librobo_hip.so -- the C ABI declared in include/robo_hip.h.

This is the binding a RoBO maintainer would add.  There is no CPU
implementation behind it: if the shared library is missing or no HIP device is visible the
first use raises :class:`RoboHipUnavailable`.

``use_library(path)`` lets the test-suite point the binding at the g++-interpreted build of
the same sources (tests/hipemu) to exercise host logic in the GPU-less build container; the
product never calls it.
"""
import atexit
import ctypes as C
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIBRARY = os.path.join(_HERE, "librobo_hip.so")
DEFAULT_DIAG_LIBRARY = os.path.join(_HERE, "librobo_hip_diag.so")   # self-checks / micro-benchmarks (not product)

OK, NOT_POSITIVE_DEFINITE, NOT_FITTED, BAD_SHAPE, RUNTIME_ERROR, BAD_ARGUMENT, NUMERIC_ERROR = range(7)
EP_MAX_NB = 64                                   # robo_ep_joint_min's cap on the representer points of one belief
EP_NAN_MESSAGE = ("an error occurs while running expectation propagation in entropy search. "
                  "Resulting variance contains NaN")
KERNEL_KINDS = {"matern52": 0, "rbf": 1, "fabolas": 2}
ACQ_KINDS = {"ei": 0, "log_ei": 1, "pi": 2, "lcb": 3}
FLAG_ZERO_SIGMA, FLAG_NEGATIVE_EI, FLAG_NAN, FLAG_NOT_FACTORED, FLAG_FROZEN = 1, 2, 4, 8, 16
SCREEN_NOT_ELIGIBLE, SCREEN_SCREENED, SCREEN_PROBE_USED, SCREEN_FELL_BACK = 0, 1, 2, 3     # robo_cand_last_screen's outcome
SCREEN_FINISH_NONE, SCREEN_FINISH_FULL, SCREEN_FINISH_LEAN = 0, 1, 2                          # robo_cand_last_screen_finish
FANTASY_KINDS = {"kriging_believer": 0, "constant_liar": 1}   # robo_acq_batch_*: how a pick's fantasy target is chosen
MES_MAX_K = 128                                  # robo_mes_*: cap on the sampled minima per model
KG_MAX_DISC = 64                                 # robo_kg_*: cap on the discretisation points of the knowledge gradient
EHVI_MAX_FRONT = 4096                            # robo_ehvi_*: cap on the points of the Pareto front
CEI_MAX_CONSTRAINTS = 16                         # robo_cei_*: cap on the constraints of constrained expected improvement
PATHS_MAX = 64                                   # robo_paths_*: cap on the sample paths of one object
PATHS_MAX_FEATURES = 4096                        # ... and on its random Fourier features
PATHS_MAX_STARTS = 1024                          # robo_paths_refine_cand: cap on n_starts (per path)
PATHS_MAX_DESCENTS = 65536                       # robo_paths_descend: cap on the descents of one call
REFINE_MAX_STARTS = 1024                         # robo_acq_refine_*: cap on n_starts
MC_MAX_NB, MC_MAX_NP, MC_MAX_NF = 64, 512, 65535   # limits of the Monte-Carlo p_min entry points (robo_pmin_mc, robo_igmc_*)

# every symbol include/robo_hip.h declares (tests check the library exports all of them)
SYMBOLS = [
    "robo_device_count", "robo_ctx_create", "robo_ctx_destroy", "robo_ctx_live_count", "robo_ctx_synchronize",
    "robo_ctx_device_name", "robo_ctx_event_record", "robo_ctx_event_elapsed_ms", "robo_ctx_set_phase_events",
    "robo_ctx_set_tuning",
    "robo_last_error_string", "robo_version_string",
    "robo_gp_create", "robo_gp_destroy", "robo_gp_set_data", "robo_gp_set_output_transform",
    "robo_gp_set_precision", "robo_theta_size",
    "robo_gp_fit", "robo_gp_loglik_batch", "robo_gp_mcmc_run", "robo_mcmc_draws", "robo_gp_fit_batch", "robo_gp_grad_loglik", "robo_gp_grad_loglik_batch",
    "robo_gp_optimize_hypers", "robo_gp_get_factor", "robo_gp_get_gram", "robo_gp_factor_cond", "robo_gp_prefetch_inverse",
    "robo_cand_create", "robo_cand_destroy", "robo_cand_set_points", "robo_cand_create_uniform", "robo_cand_get_points",
    "robo_cand_create_random", "robo_cand_create_sobol", "robo_cand_get_point", "robo_cand_workspace_chunk", "robo_cand_last_solve_kernel",
    "robo_gp_predict_cand", "robo_gp_predict", "robo_gp_predict_cov", "robo_gp_predict_grad", "robo_gp_predict_mixture_cand",
    "robo_acq_eval_cand", "robo_acq_eval", "robo_acq_eval_moments", "robo_acq_eval_marginal_cand", "robo_acq_eval_sum_cand",
    "robo_cand_last_screen", "robo_cand_last_screen_finish", "robo_cand_last_screen_first", "robo_cand_last_screen_form",
    "robo_acq_screen_bounds",
    "robo_acq_refine_cand", "robo_acq_refine_marginal_cand",
    "robo_rep_sample", "robo_rep_sample_batch",
    "robo_acq_batch_cand", "robo_acq_batch_marginal_cand", "robo_qei_batch_cand", "robo_qei_batch_marginal_cand",
    "robo_mes_eval_cand", "robo_mes_eval_marginal_cand", "robo_mes_sample_min_moments", "robo_mes_eval_moments",
    "robo_kg_eval_cand", "robo_kg_eval_marginal_cand", "robo_kg_eval_moments",
    "robo_ehvi_eval_cand", "robo_ehvi_eval_moments",
    "robo_cei_eval_cand", "robo_cei_eval_moments", "robo_cei_refine_cand",
    "robo_paths_create", "robo_paths_eval_cand", "robo_paths_destroy", "robo_paths_descend", "robo_paths_refine_cand",
    "robo_ig_eval_cand", "robo_ig_eval_per_cost_cand", "robo_ig_eval_moments", "robo_gp_cross_cov",
    "robo_ep_joint_min", "robo_pmin_mc", "robo_igmc_eval_cand", "robo_igmc_eval_moments",
    "robo_comm_create_id", "robo_comm_init", "robo_comm_destroy", "robo_comm_info", "robo_comm_allgather",
    "robo_acq_eval_cand_sharded", "robo_acq_eval_marginal_cand_sharded", "robo_ig_eval_per_cost_cand_sharded",
    "robo_multi_create", "robo_multi_destroy", "robo_multi_info", "robo_gp_set_data_multi", "robo_gp_fit_multi",
    "robo_gp_loglik_batch_multi", "robo_gp_fit_batch_multi", "robo_acq_eval_cand_multi",
    "robo_ig_eval_cand_multi", "robo_ig_eval_per_cost_cand_multi", "robo_acq_eval_marginal_cand_multi",
    "robo_gp_predict_mixture_cand_multi",
]
COMM_ID_BYTES = 128
# include/robo_hip_diag.h (librobo_hip_diag.so: tests, bench.py's roofline block, tools/)
DIAG_SYMBOLS = [
    "robo_selftest_mfma_layout", "robo_microbench_mfma_f64", "robo_microbench_mfma_f64_detail", "robo_microbench_gemm_f64",
    "robo_selftest_diag_timeline", "robo_diag_clock_sample_begin", "robo_diag_clock_sample_end",
    "robo_selftest_stretch_move", "robo_diag_cross_gram", "robo_diag_cov_rows",
]


class RoboHipUnavailable(RuntimeError):
    pass


class RoboHipError(RuntimeError):
    pass


class RoboBadShape(AssertionError):
    """ROBO_BAD_SHAPE from the library (the reference uses ``assert`` for shapes, base_model.py:68-70,76) -- its own type
    so that callers can tell the library's verdict from a Python-side assert"""


_lib = None
_lib_path = None
_diag = None
_dp = C.POINTER(C.c_double)


def _arr(a):
    return a.ctypes.data_as(_dp)


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != shape:
        raise AssertionError("expected shape %r, got %r" % (shape, a.shape))
    return a


def _handles(gps):
    """the handle array of a list of device GPs (at least one slot, so that an empty list still has an address)"""
    return (C.c_void_p * max(len(gps), 1))(*[g._h for g in gps])


def _etas(eta, S):
    """one incumbent value for all S samples, or one per sample -> (S,) contiguous fp64"""
    return _f64(np.broadcast_to(np.asarray(eta, dtype=np.float64), (S,)))


def _ensemble_head(gps, eta, marginal, *between):
    """the leading arguments of an entry point that comes in a single-model and a marginal form: (handle, [between], eta) or
    (handle array, S, [between], etas); the pointer of ``etas`` keeps its array alive (ndarray.ctypes.data_as)"""
    if not marginal:
        return (gps[0]._h,) + between + (float(eta),)
    return (_handles(gps), len(gps)) + between + (_arr(_etas(eta, len(gps))),)


class _Best(object):
    """the (max, argmax, flags) out-triple of the sweeps"""

    def __init__(self):
        self.max, self.argmax, self.flags = C.c_double(0), C.c_int64(0), C.c_uint32(0)
        self.refs = (C.byref(self.max), C.byref(self.argmax), C.byref(self.flags))

    def values(self):
        return self.max.value, self.argmax.value, self.flags.value


def use_library(path):
    """Point the binding at another build of the same C ABI (test hook)."""
    global _lib, _lib_path, _default_ctx, _diag, _extra_ctx, _multis
    _close_multis()                        # worker threads of the outgoing library end here, not at garbage collection
    _lib = None
    _diag = None
    _lib_path = path
    _default_ctx = {}
    _extra_ctx = {}
    _multis = {}


def library_path():
    return _lib_path or DEFAULT_LIBRARY


def lib():
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise RoboHipUnavailable(
            "%s not found: build it with `python -m robo_amd.build` (hipcc, gfx950). "
            "robo_amd has no CPU fallback." % path)
    try:
        L = C.CDLL(path)
    except OSError as e:
        raise RoboHipUnavailable("cannot load %s: %s" % (path, e))
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    pp = C.POINTER(vp)
    sig = {
        "robo_device_count": [C.POINTER(i32)],
        "robo_ctx_create": [i32, vp, pp],
        "robo_ctx_destroy": [vp],
        "robo_ctx_live_count": [C.POINTER(i32)],
        "robo_ctx_synchronize": [vp],
        "robo_ctx_device_name": [vp, C.c_char_p, i32],
        "robo_ctx_event_record": [vp, i32],
        "robo_ctx_event_elapsed_ms": [vp, i32, i32, C.POINTER(C.c_float)],
        "robo_ctx_set_phase_events": [vp, i32],
        "robo_ctx_set_tuning": [vp, C.c_char_p, i64],
        "robo_gp_create": [vp, i32, i32, i32, pp],
        "robo_gp_destroy": [vp],
        "robo_gp_set_data": [vp, _dp, _dp, i32],
        "robo_gp_set_output_transform": [vp, dbl, dbl],
        "robo_gp_set_precision": [vp, i32],
        "robo_theta_size": [i32, i32],
        "robo_gp_fit": [vp, _dp, dbl, _dp, C.POINTER(i32)],
        "robo_gp_loglik_batch": [vp, _dp, i32, dbl, _dp, C.POINTER(i32)],
        "robo_gp_fit_batch": [pp, i32, _dp, dbl, _dp, C.POINTER(i32)],
        "robo_mcmc_draws": [C.POINTER(C.c_uint32), C.POINTER(i32), i32, i32, _dp, C.POINTER(i32), _dp],
        "robo_gp_mcmc_run": [vp, dbl, i32, _dp, i32, i32, dbl, _dp, C.POINTER(i32), _dp, i32, _dp, _dp, _dp, _dp,
                             C.POINTER(i64)],
        "robo_gp_grad_loglik": [vp, _dp, dbl, _dp, _dp, C.POINTER(i32)],
        "robo_gp_grad_loglik_batch": [vp, _dp, i32, dbl, _dp, _dp, C.POINTER(i32)],
        "robo_gp_optimize_hypers": [vp, dbl, i32, _dp, _dp, _dp, _dp, i32, i32, i32, dbl, dbl, dbl, _dp, _dp,
                                    C.POINTER(i32), _dp, _dp, C.POINTER(i32), _dp],
        "robo_gp_get_factor": [vp, _dp],
        "robo_gp_get_gram": [vp, _dp, _dp],
        "robo_gp_factor_cond": [vp, _dp],
        "robo_gp_prefetch_inverse": [vp],
        "robo_cand_create": [vp, _dp, i64, i32, pp],
        "robo_cand_destroy": [vp],
        "robo_cand_set_points": [vp, _dp, i64],
        "robo_cand_create_uniform": [vp, i64, i32, C.c_uint64, pp],
        "robo_cand_get_points": [vp, _dp],
        "robo_cand_create_random": [vp, i64, i32, C.c_uint64, i64, _dp, _dp, pp],
        "robo_cand_create_sobol": [vp, i64, i32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), i32, C.c_uint64, pp],
        "robo_cand_get_point": [vp, i64, _dp],
        "robo_cand_workspace_chunk": [vp, C.POINTER(i64)],
        "robo_cand_last_solve_kernel": [vp, C.c_char_p, i32],
        "robo_gp_predict_cand": [vp, vp, _dp, _dp],
        "robo_gp_predict": [vp, _dp, i64, _dp, _dp],
        "robo_gp_predict_cov": [vp, _dp, i64, _dp, _dp],
        "robo_gp_predict_grad": [vp, _dp, i64, _dp, _dp, _dp, _dp],
        "robo_gp_predict_mixture_cand": [pp, i32, vp, _dp, _dp],
        "robo_acq_eval_cand": [vp, i32, dbl, dbl, vp, _dp, _dp, C.POINTER(i64), C.POINTER(C.c_uint32)],
        "robo_acq_eval": [vp, i32, dbl, dbl, _dp, i64, _dp, _dp, C.POINTER(i64), C.POINTER(C.c_uint32)],
        "robo_cand_last_screen": [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i32)],
        "robo_cand_last_screen_finish": [vp, C.POINTER(i32), C.POINTER(i32)],
        "robo_cand_last_screen_first": [vp, C.POINTER(i32), C.POINTER(i64)],
        "robo_cand_last_screen_form": [vp, C.POINTER(i32), C.POINTER(C.c_double)],
        "robo_acq_screen_bounds": [vp, i32, dbl, dbl, vp, _dp, _dp],
        "robo_acq_eval_moments": [vp, i32, dbl, dbl, _dp, _dp, i64, _dp, _dp, C.POINTER(i64), C.POINTER(C.c_uint32)],
        "robo_acq_eval_marginal_cand": [pp, i32, i32, dbl, _dp, vp, _dp, _dp, C.POINTER(i64),
                                        C.POINTER(C.c_uint32)],
        "robo_acq_eval_sum_cand": [pp, i32, i32, dbl, _dp, vp, _dp, C.POINTER(C.c_uint32)],
        "robo_acq_refine_cand": [vp, i32, dbl, dbl, vp, i32, i32, dbl, _dp, _dp, C.POINTER(i64), C.POINTER(C.c_uint32),
                                 C.POINTER(i64), _dp],
        "robo_acq_refine_marginal_cand": [pp, i32, i32, dbl, _dp, vp, i32, i32, dbl, _dp, _dp, C.POINTER(i64),
                                          C.POINTER(C.c_uint32), C.POINTER(i64), _dp],
        "robo_rep_sample": [vp, i32, dbl, dbl, _dp, _dp, i32, i32, i32, dbl, _dp, C.POINTER(i32), _dp, _dp, _dp, i32,
                            C.POINTER(i64), C.POINTER(C.c_uint32), _dp],
        "robo_rep_sample_batch": [pp, i32, i32, dbl, _dp, _dp, _dp, i32, i32, i32, dbl, _dp, C.POINTER(i32), _dp, _dp, _dp,
                                  i32, C.POINTER(i64), C.POINTER(C.c_uint32), _dp],
        "robo_acq_batch_cand": [vp, i32, dbl, dbl, vp, i32, i32, dbl, C.POINTER(i64), _dp, _dp, C.POINTER(C.c_uint32),
                                C.POINTER(i32), _dp],
        "robo_acq_batch_marginal_cand": [pp, i32, i32, dbl, _dp, vp, i32, i32, dbl, C.POINTER(i64), _dp, _dp,
                                         C.POINTER(C.c_uint32), C.POINTER(i32), _dp],
        "robo_qei_batch_cand": [vp, dbl, dbl, vp, i32, _dp, i32, C.POINTER(i64), _dp, C.POINTER(C.c_uint32), C.POINTER(i32),
                                _dp, _dp, _dp, _dp, _dp],
        "robo_qei_batch_marginal_cand": [pp, i32, dbl, _dp, vp, i32, _dp, i32, C.POINTER(i64), _dp, C.POINTER(C.c_uint32),
                                         C.POINTER(i32), _dp, _dp, _dp, _dp, _dp],
        "robo_mes_eval_cand": [vp, dbl, vp, _dp, i32, i32, _dp, _dp, C.POINTER(i64), C.POINTER(C.c_uint32), _dp, _dp, _dp],
        "robo_mes_eval_marginal_cand": [pp, i32, _dp, vp, _dp, i32, i32, _dp, _dp, C.POINTER(i64), C.POINTER(C.c_uint32),
                                        _dp, _dp, _dp],
        "robo_mes_sample_min_moments": [vp, _dp, _dp, i64, _dp, i32, i32, dbl, _dp, _dp],
        "robo_mes_eval_moments": [vp, _dp, _dp, i64, _dp, i32, _dp, _dp, C.POINTER(i64), C.POINTER(C.c_uint32)],
        "robo_kg_eval_cand": [vp, vp, vp, dbl, i32, _dp, _dp, C.POINTER(i64), C.POINTER(C.c_uint32), _dp, _dp],
        "robo_kg_eval_marginal_cand": [pp, i32, vp, vp, _dp, i32, _dp, _dp, C.POINTER(i64), C.POINTER(C.c_uint32), _dp, _dp],
        "robo_kg_eval_moments": [vp, i64, i32, dbl, i32, _dp, _dp, _dp, _dp, _dp, _dp, C.POINTER(i64),
                                 C.POINTER(C.c_uint32)],
        "robo_ehvi_eval_cand": [vp, vp, vp, _dp, i32, _dp, _dp, _dp, C.POINTER(i64), C.POINTER(C.c_uint32), _dp],
        "robo_ehvi_eval_moments": [vp, i64, _dp, _dp, _dp, _dp, _dp, i32, _dp, _dp, _dp, C.POINTER(i64),
                                   C.POINTER(C.c_uint32)],
        "robo_cei_eval_cand": [vp, pp, i32, _dp, i32, dbl, dbl, i32, vp, _dp, _dp, C.POINTER(i64), C.POINTER(C.c_uint32),
                               _dp],
        "robo_cei_eval_moments": [vp, i64, i32, _dp, _dp, _dp, _dp, _dp, i32, dbl, dbl, i32, _dp, _dp, C.POINTER(i64),
                                  C.POINTER(C.c_uint32)],
        "robo_cei_refine_cand": [vp, pp, i32, _dp, i32, dbl, dbl, i32, vp, i32, i32, dbl, _dp, _dp, C.POINTER(i64),
                                 C.POINTER(C.c_uint32), C.POINTER(i64), _dp],
        "robo_paths_create": [vp, i32, i32, _dp, _dp, _dp, _dp, pp],
        "robo_paths_eval_cand": [vp, vp, _dp, _dp, C.POINTER(i64), C.POINTER(C.c_uint32)],
        "robo_paths_destroy": [vp],
        "robo_paths_descend": [vp, i32, C.POINTER(i32), _dp, i32, dbl, _dp, _dp, _dp, C.POINTER(i32), C.POINTER(C.c_uint32),
                               _dp],
        "robo_paths_refine_cand": [vp, vp, i32, i32, dbl, _dp, _dp, C.POINTER(i64), C.POINTER(C.c_uint32), C.POINTER(i64),
                                   _dp],
        "robo_ig_eval_cand": [vp, vp, vp, i32, dbl, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.POINTER(i64)],
        "robo_ig_eval_per_cost_cand": [vp, vp, vp, i32, dbl, _dp, _dp, _dp, _dp, _dp, _dp, vp, vp, dbl, _dp, _dp,
                                       C.POINTER(i64)],
        "robo_ig_eval_per_cost_cand_sharded": [vp, vp, vp, vp, i32, dbl, _dp, _dp, _dp, _dp, _dp, _dp, vp, vp, dbl, i64,
                                               _dp, _dp, C.POINTER(i64), C.POINTER(i32)],
        "robo_ig_eval_moments": [vp, i64, i32, i32, dbl, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp],
        "robo_gp_cross_cov": [vp, vp, vp, _dp],
        "robo_ep_joint_min": [vp, i32, i32, _dp, _dp, i32, _dp, _dp, _dp, _dp, C.POINTER(i32), C.POINTER(i32)],
        "robo_pmin_mc": [vp, i32, i32, i32, _dp, _dp, _dp, _dp, _dp, C.POINTER(i32)],
        "robo_igmc_eval_cand": [vp, vp, vp, i32, i32, dbl, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.POINTER(i64),
                                C.POINTER(C.c_uint32)],
        "robo_igmc_eval_moments": [vp, i64, i32, i32, i32, dbl, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                   C.POINTER(i32), _dp],
        "robo_comm_create_id": [C.c_char_p],
        "robo_comm_init": [vp, i32, i32, C.c_char_p, pp],
        "robo_comm_destroy": [vp],
        "robo_comm_info": [vp, C.POINTER(i32), C.POINTER(i32)],
        "robo_comm_allgather": [vp, _dp, i64, _dp],
        "robo_acq_eval_cand_sharded": [vp, vp, i32, dbl, dbl, vp, i64, _dp, _dp, C.POINTER(i64), C.POINTER(i32),
                                       C.POINTER(C.c_uint32)],
        "robo_acq_eval_marginal_cand_sharded": [vp, pp, i32, i32, i32, dbl, _dp, vp, _dp, _dp, C.POINTER(i64),
                                                C.POINTER(C.c_uint32)],
        "robo_multi_create": [pp, i32, pp],
        "robo_multi_destroy": [vp],
        "robo_multi_info": [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)],
        "robo_gp_set_data_multi": [vp, pp, _dp, _dp, i32],
        "robo_gp_fit_multi": [vp, pp, _dp, dbl, _dp, C.POINTER(i32)],
        "robo_gp_loglik_batch_multi": [vp, pp, _dp, i32, dbl, _dp, C.POINTER(i32)],
        "robo_gp_fit_batch_multi": [vp, pp, C.POINTER(i32), _dp, dbl, _dp, C.POINTER(i32)],
        "robo_acq_eval_cand_multi": [vp, pp, i32, dbl, dbl, pp, C.POINTER(i64), _dp, _dp, C.POINTER(i64), C.POINTER(i32),
                                     C.POINTER(C.c_uint32)],
        "robo_ig_eval_cand_multi": [vp, pp, pp, pp, i32, dbl, _dp, _dp, _dp, _dp, _dp, _dp, C.POINTER(i64), _dp, _dp,
                                    C.POINTER(i64), C.POINTER(i32)],
        "robo_ig_eval_per_cost_cand_multi": [vp, pp, pp, pp, i32, dbl, _dp, _dp, _dp, _dp, _dp, _dp, pp, pp, dbl,
                                             C.POINTER(i64), _dp, _dp, C.POINTER(i64), C.POINTER(i32)],
        "robo_acq_eval_marginal_cand_multi": [vp, pp, C.POINTER(i32), i32, dbl, _dp, pp, _dp, _dp, C.POINTER(i64),
                                              C.POINTER(C.c_uint32)],
        "robo_gp_predict_mixture_cand_multi": [vp, pp, C.POINTER(i32), pp, _dp, _dp],
    }
    for name, args in sig.items():
        if path != DEFAULT_LIBRARY and not hasattr(L, name):
            # a build given through use_library (bench.py --lib: an A/B build of another commit) may lack an entry point of
            # this binding: it loads, and the call says so.  The product library must export every one (build() checks it)
            def missing(*_, _name=name, _path=path):
                raise RoboHipUnavailable("%s does not export %s" % (_path, _name))
            setattr(L, name, missing)
            continue
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = i32
    L.robo_last_error_string.restype = C.c_char_p
    L.robo_last_error_string.argtypes = []
    L.robo_version_string.restype = C.c_char_p
    L.robo_version_string.argtypes = []
    n = i32(0)
    L.robo_device_count(C.byref(n))
    if n.value < 1:
        raise RoboHipUnavailable("librobo_hip loaded but no HIP device is visible (robo_amd has no CPU fallback)")
    _lib = L
    return L


def diag():
    """the diagnostics library (self-checks, micro-benchmarks); the interpreter build of the tests is monolithic"""
    global _diag
    if _diag is not None:
        return _diag
    lib()                                            # the product library first (the diagnostics link against it)
    path = _lib_path or DEFAULT_DIAG_LIBRARY
    if not os.path.exists(path):
        raise RoboHipUnavailable("%s not found: build it with `python -m robo_amd.build`" % path)
    D = C.CDLL(path)
    vp, i32 = C.c_void_p, C.c_int32
    for name, args in {"robo_selftest_mfma_layout": [vp, _dp], "robo_microbench_mfma_f64": [vp, i32, _dp],
                       "robo_microbench_mfma_f64_detail": [vp, i32, _dp],
                       "robo_microbench_gemm_f64": [vp, i32, i32, i32, i32, _dp],
                       "robo_selftest_diag_timeline": [vp, _dp, _dp],
                       "robo_diag_clock_sample_begin": [vp, i32], "robo_diag_clock_sample_end": [vp, _dp],
                       "robo_selftest_stretch_move": [vp, _dp, _dp, _dp, C.c_double, i32, i32, _dp, _dp, _dp],
                       "robo_diag_cross_gram": [vp, _dp, _dp, i32, _dp],
                       "robo_diag_cov_rows": [vp, i32, i32, C.c_double, C.c_double, C.c_double, _dp, _dp, C.c_int64,
                                              _dp]}.items():
        fn = getattr(D, name)
        fn.argtypes = args
        fn.restype = i32
    _diag = D
    return D


def last_error():
    return lib().robo_last_error_string().decode("utf-8", "replace")


def check(status, msg=None):
    """Map a robo_status to the exception the reference raises at the same point.  msg: the text to use instead of the
    library's last error string (a status that arrived from ANOTHER rank has no local error string)."""
    if status == OK:
        return
    msg = last_error() if msg is None else msg
    if status == NOT_POSITIVE_DEFINITE:
        raise np.linalg.LinAlgError(msg or "matrix is not positive definite")
    if status == NOT_FITTED:
        raise Exception('Model has to be trained first!')    # gaussian_process.py:241,273,322
    if status == BAD_SHAPE:
        raise RoboBadShape(msg)                               # base_model.py:68-70,76 use assert
    if status == BAD_ARGUMENT:
        raise ValueError(msg)
    if status == NUMERIC_ERROR:
        raise Exception(EP_NAN_MESSAGE)                       # robo/util/epmgp.py (the EP working covariance)
    raise RoboHipError(msg)


def live_contexts():
    """contexts whose device resources are still held by the library (robo_ctx_live_count)"""
    n = C.c_int32(0)
    lib().robo_ctx_live_count(C.byref(n))
    return n.value


def device_count():
    n = C.c_int32(0)
    lib().robo_device_count(C.byref(n))
    return n.value


def mcmc_draws(random_state, n_steps, half):
    """(u_stretch, partner, u_accept), each (n_steps, 2, half): the numbers `random_state` (a legacy numpy RandomState)
    would produce for n_steps emcee-2 ensemble steps -- rand(half), randint(half, size=half), rand(half) per half-step --
    drawn by the library (robo_mcmc_draws) and with the stream advanced exactly as those calls would have advanced it."""
    name, key, pos, has_gauss, cached = random_state.get_state()
    if name != "MT19937":
        raise ValueError("legacy MT19937 RandomState expected")
    key = np.ascontiguousarray(key, dtype=np.uint32).copy()
    p = C.c_int32(int(pos))
    uz = np.empty((n_steps, 2, half))
    ua = np.empty((n_steps, 2, half))
    pa = np.empty((n_steps, 2, half), dtype=np.int32)
    check(lib().robo_mcmc_draws(key.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(p), int(n_steps), int(half), _arr(uz),
                                pa.ctypes.data_as(C.POINTER(C.c_int32)), _arr(ua)))
    random_state.set_state((name, key, int(p.value), has_gauss, cached))
    return uz, pa, ua


class Context(object):
    """robo_ctx: one device, one HIP stream, 34 event slots."""

    def __init__(self, device=0, stream=None):
        self._h = C.c_void_p()
        self._owner = lib()          # the library that owns the handle (tests switch libraries: use_library)
        check(self._owner.robo_ctx_create(int(device), C.c_void_p(stream) if stream else None, C.byref(self._h)))
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._owner.robo_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        check(lib().robo_ctx_synchronize(self._h))

    @property
    def name(self):
        buf = C.create_string_buffer(256)
        check(lib().robo_ctx_device_name(self._h, buf, 256))
        return buf.value.decode()

    def record(self, slot):
        check(lib().robo_ctx_event_record(self._h, int(slot)))

    def elapsed_ms(self, a, b):
        ms = C.c_float(0)
        check(lib().robo_ctx_event_elapsed_ms(self._h, int(a), int(b), C.byref(ms)))
        return float(ms.value)

    def set_phase_events(self, on):
        """record event slots 19..23 around the phases of robo_gp_fit (off by default)"""
        check(lib().robo_ctx_set_phase_events(self._h, 1 if on else 0))

    def set_tuning(self, key, value=None):
        """kernel-variant / workspace knobs of this context (include/robo_hip.h); value None restores the default,
        key "env" re-reads the ROBO_* environment variables"""
        v = -(2 ** 63) if value is None else int(value)
        check(lib().robo_ctx_set_tuning(self._h, key.encode(), v))

    def selftest_mfma_layout(self):
        e = C.c_double(0)
        check(diag().robo_selftest_mfma_layout(self._h, C.byref(e)))
        return e.value

    def selftest_stretch_move(self, c, s, u, a=2.0, P=18):
        """-> (z, q, lnpdiff) of the chain's stretch-move device functions on arrays (include/robo_hip_diag.h)"""
        c, s, u = (np.ascontiguousarray(v, dtype=np.float64) for v in (c, s, u))
        assert c.shape == s.shape == u.shape and c.ndim == 1
        z, q, d = np.empty_like(c), np.empty_like(c), np.empty_like(c)
        check(diag().robo_selftest_stretch_move(self._h, _arr(c), _arr(s), _arr(u), float(a), int(P), c.size,
                                                _arr(z), _arr(q), _arr(d)))
        return z, q, d

    def cov_rows(self, kind, xi, xj, amp=1.0, blr_a=0.0, blr_b=0.0):
        """-> the device function cov_rows on pairs of already scaled rows xi, xj (n, dim) (include/robo_hip_diag.h)"""
        xi, xj = _f64(xi), _f64(xj)
        assert xi.ndim == 2 and xi.shape == xj.shape
        out = np.empty(xi.shape[0])
        check(diag().robo_diag_cov_rows(self._h, KERNEL_KINDS[kind], xi.shape[1], float(amp), float(blr_a), float(blr_b),
                                        _arr(xi), _arr(xj), xi.shape[0], _arr(out)))
        return out

    def microbench_mfma_f64_detail(self, iters=2000):
        """-> dict(full-chip tflops, issue interval of one lone wave in shader cycles, MHz under load)"""
        out = np.zeros(4)
        check(diag().robo_microbench_mfma_f64_detail(self._h, int(iters), _arr(out)))
        return {"tflops": out[0], "cycles_per_mfma_single_wave": out[1], "shader_mhz": out[2],
                "cycles_per_mfma_dependent_chain": out[3]}

    def microbench_gemm_f64(self, variant, wgs=512, k=4096, reps=5):
        out = np.zeros(2)
        check(diag().robo_microbench_gemm_f64(self._h, int(variant), int(wgs), int(k), int(reps), _arr(out)))
        return float(out[0]), float(out[1])    # TFLOP/s, shader MHz

    def clock_sample_begin(self, window_us):
        """Shader-clock sampler on a private stream (include/robo_hip_diag.h); measurement only."""
        check(diag().robo_diag_clock_sample_begin(self._h, int(window_us)))

    def clock_sample_end(self):
        out = np.zeros(3)
        check(diag().robo_diag_clock_sample_end(self._h, _arr(out)))
        return {"mean": float(out[0]), "min": float(out[1]), "max": float(out[2])}

    def microbench_mfma_f64(self, iters=2000):
        t = C.c_double(0)
        check(diag().robo_microbench_mfma_f64(self._h, int(iters), C.byref(t)))
        return t.value


_default_ctx = {}


def default_context(device=None):
    if device is None:
        device = int(os.environ.get("ROBO_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        if device >= device_count():
            device = 0
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


_extra_ctx = {}        # (device, k): the k-th additional context on a device that appears more than once in a device list
_multis = {}           # tuple(devices) -> Multi
_live_multis = weakref.WeakSet()


def _close_multis():
    """End every Multi's worker threads while the interpreter and the HIP runtime are fully alive.  Registered with atexit:
    left to garbage collection during interpreter finalisation, the join of a worker thread (whose exit runs the HIP
    runtime's thread-local destructors) was seen to hang or abort the process on the MI355X (r05: a test process whose last
    test had used a device list)."""
    for m in list(_live_multis):
        try:
            m.close()
        except Exception:      # noqa: BLE001
            pass
    _multis.clear()


atexit.register(_close_multis)


def resolve_devices(devices=None, n_gpus=None):
    """the device list of a single-process multi-device run, or None for the ordinary one-device case:
    ``devices`` = explicit HIP device ids (a device may appear twice: two contexts on it, for tests on a one-GPU box),
    ``n_gpus`` = G -> devices 0 .. G-1"""
    if devices is None and n_gpus is not None and int(n_gpus) > 1:
        devices = list(range(int(n_gpus)))
    if devices is None:
        return None
    devices = [int(d) for d in devices]
    n = device_count()
    if any(d < 0 or d >= n for d in devices):
        raise ValueError("devices %r: this process sees %d HIP device(s)" % (devices, n))
    return devices if len(devices) > 1 else None


def contexts_for(devices):
    """one Context per entry of ``devices``: the process-wide default context of a device for its first occurrence, an
    extra one (kept for the life of the process) for every further occurrence"""
    seen = {}
    out = []
    for d in devices:
        k = seen.get(d, 0)
        seen[d] = k + 1
        if k == 0:
            out.append(default_context(d))
        else:
            if (d, k) not in _extra_ctx:
                _extra_ctx[(d, k)] = Context(d)
            out.append(_extra_ctx[(d, k)])
    return out


def multi_for(devices):
    """the process-wide Multi of a device list (every model / acquisition function given the same list shares it)"""
    key = tuple(int(d) for d in devices)
    if key not in _multis:
        _multis[key] = Multi(contexts_for(key))
    return _multis[key]


def shard_range(n_items, slot, n_slots):
    """contiguous [begin, end) of a slot's shard; the first n_items % n_slots slots hold one more (the library's rule)"""
    base, rem = divmod(int(n_items), int(n_slots))
    begin = slot * base + min(slot, rem)
    return begin, begin + base + (1 if slot < rem else 0)


class Candidates(object):
    """robo_cand: a device-resident candidate batch (normalised input space) + workspace."""

    def __init__(self, ctx, Xc=None, m=None, dim=None, seed=None, n_uniform=None, loc=None, scale=None, sobol=None,
                 first=0):
        self.ctx = ctx
        self._h = C.c_void_p()
        self._owner = lib()
        if sobol is not None:
            # sobol: a scipy.stats.qmc.Sobol engine (its direction numbers and digital shift are read, the engine is
            # not advanced) or a (sv (dim, bits), shift (dim,), bits) triple; points first .. first + m - 1
            if hasattr(sobol, "random"):          # a scipy.stats.qmc.Sobol engine
                if not all(hasattr(sobol, a) for a in ("_sv", "_shift", "bits")):
                    raise RoboHipError("this SciPy's qmc.Sobol does not expose its direction numbers (_sv, _shift, "
                                       "bits; SciPy 1.7-1.15 do): pass a (sv, shift, bits) triple instead")
                sv, shift, bits = sobol._sv, sobol._shift, int(sobol.bits)
            else:
                sv, shift, bits = sobol
            sv = np.ascontiguousarray(sv, dtype=np.uint64)
            shift = np.ascontiguousarray(shift, dtype=np.uint64)
            assert sv.ndim == 2 and sv.shape[1] == bits and shift.shape == (sv.shape[0],)
            self.m, self.dim = int(m), int(sv.shape[0])
            u64p = C.POINTER(C.c_uint64)
            check(lib().robo_cand_create_sobol(ctx._h, self.m, self.dim, sv.ctypes.data_as(u64p),
                                               shift.ctypes.data_as(u64p), bits, int(first), C.byref(self._h)))
        elif loc is not None:
            loc, scale = _f64(loc), _f64(scale)
            self.m, self.dim = int(m), int(loc.shape[0])
            assert scale.shape == loc.shape
            check(lib().robo_cand_create_random(ctx._h, self.m, self.dim, int(seed or 0),
                                                self.m if n_uniform is None else int(n_uniform), _arr(loc),
                                                _arr(scale), C.byref(self._h)))
        elif Xc is not None:
            Xc = _f64(Xc)
            assert Xc.ndim == 2
            self.m, self.dim = Xc.shape
            check(lib().robo_cand_create(ctx._h, _arr(Xc), self.m, self.dim, C.byref(self._h)))
        else:
            self.m, self.dim = int(m), int(dim)
            check(lib().robo_cand_create_uniform(ctx._h, self.m, self.dim, int(seed or 0), C.byref(self._h)))

    def set_points(self, Xc):
        """upload a new batch of the same shape into this handle (H2D only)"""
        Xc = _f64(Xc, (self.m, self.dim))
        check(lib().robo_cand_set_points(self._h, _arr(Xc), self.m))

    def point(self, index):
        out = np.empty(self.dim)
        check(lib().robo_cand_get_point(self._h, int(index), _arr(out)))
        return out

    def chunk(self):
        """candidates per workspace pass of the last posterior evaluated on this handle (0: none yet)"""
        n = C.c_int64(0)
        check(lib().robo_cand_workspace_chunk(self._h, C.byref(n)))
        return int(n.value)

    def solve_kernel(self):
        """name of the kernel that ran the solve of the last posterior evaluated on this handle"""
        buf = C.create_string_buffer(64)
        check(lib().robo_cand_last_solve_kernel(self._h, buf, 64))
        return buf.value.decode()

    def bounds_kernel(self):
        """name of the kernel that ran the last bounds pass of the acquisition screen on this handle ("": none yet): the
        second string robo_cand_last_solve_kernel leaves behind the first one's terminator"""
        buf = C.create_string_buffer(128)
        check(lib().robo_cand_last_solve_kernel(self._h, buf, 128))
        return buf.raw.split(b"\0")[1].decode()

    def screen_finish(self):
        """how the last bounds pass of the acquisition screen on this handle finished its covariances: a SCREEN_FINISH_* value"""
        f = C.c_int32(0)
        check(lib().robo_cand_last_screen_finish(self._h, C.byref(f), None))
        return int(f.value)

    def screen_tail_fused(self):
        """whether the last argmax-only acquisition call on this handle ran its survivors' tail as the one fused launch"""
        f, t = C.c_int32(0), C.c_int32(0)
        check(lib().robo_cand_last_screen_finish(self._h, C.byref(f), C.byref(t)))
        return bool(t.value)

    def screen_first(self):
        """the single-precision first stage of the last argmax-only acquisition call on this handle -> (stage, survivors):
        stage 0 it did not run, 1 it decided the call, 2 it ran and the fp64 pass followed"""
        stage, kept = C.c_int32(0), C.c_int64(0)
        check(lib().robo_cand_last_screen_first(self._h, C.byref(stage), C.byref(kept)))
        return int(stage.value), int(kept.value)

    def screen_form(self):
        """how that first stage formed its squared distances -> (SCREEN_FORM_* value, grid step in scaled coordinates; 0.0
        with SCREEN_FORM_FP64)"""
        form, step = C.c_int32(0), C.c_double(0.0)
        check(lib().robo_cand_last_screen_form(self._h, C.byref(form), C.byref(step)))
        return int(form.value), float(step.value)

    def last_screen(self):
        """what the last argmax-only acquisition call on this handle did -> (candidates screened, survivors, SCREEN_* outcome)"""
        n, kept, outcome = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        check(lib().robo_cand_last_screen(self._h, C.byref(n), C.byref(kept), C.byref(outcome)))
        return int(n.value), int(kept.value), int(outcome.value)

    def points(self):
        out = np.empty((self.m, self.dim))
        check(lib().robo_cand_get_points(self._h, _arr(out)))
        return out

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._owner.robo_cand_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _full_theta(gp, theta):
    """the hyper-parameter vector(s) the library takes, from what the caller holds: ``gp.fixed_head`` in front.  A george
    kernel WITHOUT an amplitude factor has no amplitude parameter (``Matern52Kernel(metric, ndim)`` alone: len = D; with
    ``amp * kernel`` in front: 1 + D) -- the library's vector always starts with log amp, which such a caller pins at 0."""
    head = gp.fixed_head
    if not head:
        return theta
    theta = np.asarray(theta, dtype=np.float64)
    if theta.ndim == 1:
        return np.concatenate([head, theta])
    return np.hstack([np.tile(np.asarray(head, dtype=np.float64), (theta.shape[0], 1)), theta])


class DeviceGP(object):
    """robo_gp: training data + Cholesky factor + z resident on the device."""

    def __init__(self, ctx, kind, n_max, dim, fixed_head=()):
        self.ctx, self.kind, self.n_max, self.dim = ctx, kind, int(n_max), int(dim)
        self._h = C.c_void_p()
        self._owner = lib()
        check(self._owner.robo_gp_create(ctx._h, KERNEL_KINDS[kind], self.n_max, self.dim, C.byref(self._h)))
        self.n = 0
        self.n_theta = lib().robo_theta_size(KERNEL_KINDS[kind], self.dim)
        # leading library hyper-parameters the caller does not hold (see _full_theta); () for every kernel with an amplitude
        self.fixed_head = tuple(float(v) for v in fixed_head)

    def set_precision(self, fp32_gram):
        check(lib().robo_gp_set_precision(self._h, 1 if fp32_gram else 0))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._owner.robo_gp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_data(self, X, y):
        X, y = _f64(X), _f64(y)
        assert X.ndim == 2 and y.ndim == 1 and X.shape[0] == y.shape[0] and X.shape[1] == self.dim
        check(lib().robo_gp_set_data(self._h, _arr(X), _arr(y), X.shape[0]))
        self.n = X.shape[0]

    def set_output_transform(self, y_mean, y_std):
        check(lib().robo_gp_set_output_transform(self._h, float(y_mean), float(y_std)))

    def fit(self, theta, mean_c):
        """-> log-likelihood; raises np.linalg.LinAlgError when K is not PD."""
        theta = _f64(_full_theta(self, theta), (self.n_theta,))
        ll, col = C.c_double(0), C.c_int32(0)
        check(lib().robo_gp_fit(self._h, _arr(theta), float(mean_c), C.byref(ll), C.byref(col)))
        return ll.value

    def grad_loglik(self, theta, mean_c):
        """(log likelihood, d loglik / d theta) at theta; the GP is fitted at theta afterwards.  The last
        gradient entry is d / d sigma^2, as in the reference's grad_nll (include/robo_hip.h)."""
        theta = _f64(_full_theta(self, theta), (self.n_theta,))
        ll = C.c_double()
        col = C.c_int32()
        grad = np.empty(self.n_theta)
        check(lib().robo_gp_grad_loglik(self._h, _arr(theta), float(mean_c), C.byref(ll), _arr(grad), C.byref(col)))
        return ll.value, grad[len(self.fixed_head):]

    def loglik_batch(self, thetas, mean_c):
        thetas = _f64(_full_theta(self, np.atleast_2d(thetas)))
        assert thetas.ndim == 2 and thetas.shape[1] == self.n_theta
        S = thetas.shape[0]
        ll = np.empty(S)
        st = np.empty(S, dtype=np.int32)
        check(lib().robo_gp_loglik_batch(self._h, _arr(thetas), S, float(mean_c), _arr(ll),
                                         st.ctypes.data_as(C.POINTER(C.c_int32))))
        return ll, st

    def grad_loglik_batch(self, thetas, mean_c):
        """S (log likelihood, gradient) pairs in one batched pass (robo_gp_grad_loglik_batch) -> (ll (S), grad (S, P),
        status (S)); per sample :meth:`grad_loglik`'s bits.  The GP is left unfitted."""
        thetas = _f64(_full_theta(self, np.atleast_2d(thetas)))
        assert thetas.ndim == 2 and thetas.shape[1] == self.n_theta
        S = thetas.shape[0]
        ll = np.empty(S)
        grad = np.empty((S, self.n_theta))
        st = np.empty(S, dtype=np.int32)
        check(lib().robo_gp_grad_loglik_batch(self._h, _arr(thetas), S, float(mean_c), _arr(ll), _arr(grad),
                                              st.ctypes.data_as(C.POINTER(C.c_int32))))
        return ll, grad[:, len(self.fixed_head):], st

    def optimize_hypers(self, mean_c, prior, lower, upper, starts, n_iters=60, history=8, step0=0.5, c1=1e-4, gtol=1e-5,
                        diagnostics=False):
        """Multi-start MAP optimisation of the hyper-parameters on the device (robo_gp_optimize_hypers): prior as in
        :meth:`mcmc_run`; lower / upper (P) the box; starts (n_starts, P).  -> HyperOptResult"""
        assert not self.fixed_head, "the device optimiser moves every library hyper-parameter: use the host optimiser"
        P = self.n_theta
        starts = _f64(np.atleast_2d(starts))
        K = starts.shape[0]
        assert starts.shape == (K, P)
        lower, upper = _f64(np.broadcast_to(lower, (P,))), _f64(np.broadcast_to(upper, (P,)))
        if prior is None:
            kind, par = 0, np.zeros(9)
        else:                                    # (kind, 5 parameters) DefaultPrior / (kind, 9 parameters) EnvPrior
            kind = int(prior[0])
            par = np.zeros(9)
            given = _f64(prior[1]).reshape(-1)
            assert given.size == (9 if kind == 2 else 5)
            par[:given.size] = given
        n_iters = int(n_iters)
        theta, value, best = np.empty(P), C.c_double(), C.c_int32()
        final, values, status = np.empty((K, P)), np.empty(K), np.empty(K, dtype=np.int32)
        trace = np.empty((max(n_iters, 0) + 1, K, 2 * P + 3)) if diagnostics else None
        check(lib().robo_gp_optimize_hypers(self._h, float(mean_c), kind, _arr(par), _arr(lower), _arr(upper), _arr(starts),
                                            K, n_iters, int(history), float(step0), float(c1), float(gtol), _arr(theta),
                                            C.byref(value), C.byref(best), _arr(final), _arr(values),
                                            status.ctypes.data_as(C.POINTER(C.c_int32)),
                                            _arr(trace) if diagnostics else None))
        return HyperOptResult(theta, value.value, best.value, final, values, status, trace)

    def mcmc_run(self, mean_c, prior, pos, lnp, n_steps, u_stretch, partner, u_accept, a=2.0):
        """emcee 2's EnsembleSampler.run_mcmc on the device (robo_gp_mcmc_run): prior = None, (1, 5 parameters) DefaultPrior or
        (2, 9 parameters) EnvPrior;
        lnp None = evaluate the start positions.  -> (pos, lnp, chain (k, n_steps, P), lnprob (k, n_steps), accepted (k))"""
        pos = np.array(pos, dtype=np.float64, order="C")
        k = pos.shape[0]
        assert not self.fixed_head, "the device chain moves every library hyper-parameter: use the host sampler"
        assert pos.shape == (k, self.n_theta)
        eval_start = lnp is None
        lnp = np.zeros(k) if eval_start else np.array(lnp, dtype=np.float64)
        n_steps = int(n_steps)
        uz = np.ascontiguousarray(u_stretch, dtype=np.float64).reshape(-1)
        ua = np.ascontiguousarray(u_accept, dtype=np.float64).reshape(-1)
        pa = np.ascontiguousarray(partner, dtype=np.int32).reshape(-1)
        assert uz.size == ua.size == pa.size == n_steps * k
        chain = np.empty((k, n_steps, self.n_theta))
        lnps = np.empty((k, n_steps))
        acc = np.zeros(k, dtype=np.int64)
        if prior is None:
            kind, par = 0, np.zeros(9)
        else:                                    # (kind, 5 parameters) DefaultPrior / (kind, 9 parameters) EnvPrior
            kind = int(prior[0])
            par = np.zeros(9)
            given = _f64(prior[1]).reshape(-1)
            assert given.size == (9 if kind == 2 else 5)
            par[:given.size] = given
        check(lib().robo_gp_mcmc_run(self._h, float(mean_c), kind, _arr(par), k, n_steps, float(a), _arr(uz),
                                     pa.ctypes.data_as(C.POINTER(C.c_int32)), _arr(ua), int(eval_start), _arr(pos),
                                     _arr(lnp), _arr(chain), _arr(lnps), acc.ctypes.data_as(C.POINTER(C.c_int64))))
        return pos, lnp, chain, lnps, acc

    def factor(self):
        out = np.empty((self.n, self.n))
        check(lib().robo_gp_get_factor(self._h, _arr(out)))
        return out

    def prefetch_inverse(self):
        """start building W = L^-1 for small candidate batches now, asynchronously (robo_gp_prefetch_inverse)"""
        check(lib().robo_gp_prefetch_inverse(self._h))

    def factor_cond(self):
        """(cond_inf(L) -- exact, from the explicit inverse --, min L_ii, max L_ii) of the current factor"""
        out = np.zeros(3)
        check(lib().robo_gp_factor_cond(self._h, _arr(out)))
        return float(out[0]), float(out[1]), float(out[2])

    def gram(self, theta):
        theta = _f64(_full_theta(self, theta), (self.n_theta,))
        out = np.empty((self.n, self.n))
        check(lib().robo_gp_get_gram(self._h, _arr(theta), _arr(out)))
        return out

    def cross_gram(self, theta, Xc):
        """-> (m, n) the posterior's cross-gram kernel at theta against candidates Xc (include/robo_hip_diag.h)"""
        theta = _f64(_full_theta(self, theta), (self.n_theta,))
        Xc = _f64(Xc)
        assert Xc.ndim == 2 and Xc.shape[1] == self.dim
        out = np.empty((Xc.shape[0], self.n))
        check(diag().robo_diag_cross_gram(self._h, _arr(theta), _arr(Xc), Xc.shape[0], _arr(out)))
        return out

    def diag_timeline(self, theta):
        theta = _f64(theta, (self.n_theta,))
        out = np.zeros(38)
        check(diag().robo_selftest_diag_timeline(self._h, _arr(theta), _arr(out)))
        return out

    def predict(self, Xc):
        if isinstance(Xc, Candidates):
            mean, var = np.empty(Xc.m), np.empty(Xc.m)
            check(lib().robo_gp_predict_cand(self._h, Xc._h, _arr(mean), _arr(var)))
            return mean, var
        Xc = _f64(Xc)
        assert Xc.ndim == 2 and Xc.shape[1] == self.dim
        mean, var = np.empty(Xc.shape[0]), np.empty(Xc.shape[0])
        check(lib().robo_gp_predict(self._h, _arr(Xc), Xc.shape[0], _arr(mean), _arr(var)))
        return mean, var

    def predict_cov(self, Xc):
        Xc = _f64(Xc)
        assert Xc.ndim == 2 and Xc.shape[1] == self.dim
        m = Xc.shape[0]
        mean, cov = np.empty(m), np.empty((m, m))
        check(lib().robo_gp_predict_cov(self._h, _arr(Xc), m, _arr(mean), _arr(cov)))
        return mean, cov

    def predict_grad(self, Xc):
        """-> (mean (M,), var (M,), d mean / d x (M, D), d var / d x (M, D)) in the GP's input space"""
        Xc = _f64(Xc)
        assert Xc.ndim == 2 and Xc.shape[1] == self.dim
        m = Xc.shape[0]
        mean, var, dm, dv = np.empty(m), np.empty(m), np.empty((m, self.dim)), np.empty((m, self.dim))
        check(lib().robo_gp_predict_grad(self._h, _arr(Xc), m, _arr(mean), _arr(var), _arr(dm), _arr(dv)))
        return mean, var, dm, dv

    def acq(self, kind, par, eta, Xc, want_values=True):
        """-> (values or None, max, argmax, flags)"""
        best = _Best()
        if isinstance(Xc, Candidates):
            m = Xc.m
            out = np.empty(m) if want_values else None
            check(lib().robo_acq_eval_cand(self._h, ACQ_KINDS[kind], float(par), float(eta), Xc._h,
                                           _arr(out) if want_values else None, *best.refs))
        else:
            Xc = _f64(Xc)
            assert Xc.ndim == 2 and Xc.shape[1] == self.dim
            m = Xc.shape[0]
            out = np.empty(m) if want_values else None
            check(lib().robo_acq_eval(self._h, ACQ_KINDS[kind], float(par), float(eta), _arr(Xc), m,
                                      _arr(out) if want_values else None, *best.refs))
        return (out,) + best.values()

    def screen_bounds(self, kind, par, eta, cand):
        """-> (upper, lower) bounds of the acquisition value of every candidate, as the screen of argmax-only calls forms them"""
        up, lo = np.empty(cand.m), np.empty(cand.m)
        check(lib().robo_acq_screen_bounds(self._h, ACQ_KINDS[kind], float(par), float(eta), cand._h, _arr(up), _arr(lo)))
        return up, lo

    def refine(self, kind, par, eta, cand, n_starts=256, n_steps=50, step0=0.05, diagnostics=False):
        """sweep over ``cand`` + multi-start projected gradient ascent on the device (robo_acq_refine_cand)
        -> RefineResult; see :func:`acq_refine`"""
        return acq_refine([self], kind, par, eta, cand, n_starts, n_steps, step0, diagnostics, marginal=False)


    def select_batch(self, kind, par, eta, cand, q, fantasy="kriging_believer", liar=0.0, diagnostics=False):
        """q greedy picks from ``cand`` with fantasised observations in between (robo_acq_batch_cand) -> BatchResult;
        see :func:`acq_batch`"""
        return acq_batch([self], kind, par, eta, cand, q, fantasy, liar, diagnostics, marginal=False)

    def select_batch_joint(self, par, eta, cand, q, z, diagnostics=False):
        """q greedy picks from ``cand`` by joint Monte-Carlo batch EI over the base samples z (K, q) (robo_qei_batch_cand)
        -> QEIResult; see :func:`qei_batch`"""
        return qei_batch([self], par, eta, cand, q, z, diagnostics, marginal=False)


    def mes(self, eta, cand, u, clamp=True, want_values=True, diagnostics=False):
        """max-value entropy search over ``cand`` with the caller's uniforms u (K,) (robo_mes_eval_cand) -> MESResult;
        see :func:`mes_marginal`"""
        return mes_marginal([self], eta, cand, u, clamp, want_values, diagnostics, marginal=False)


    def kg(self, cand, rep, sn2, include_self=True, want_values=True, diagnostics=False):
        """knowledge gradient of ``cand`` over the discretisation ``rep`` (robo_kg_eval_cand) -> KGResult; see
        :func:`kg_marginal`"""
        return kg_marginal([self], cand, rep, sn2, include_self, want_values, diagnostics, marginal=False)


    def ehvi(self, other, cand, front, ref, want_values=True, diagnostics=False):
        """two-objective expected hypervolume improvement of ``cand`` with this GP as the first objective and ``other``
        as the second, over the sorted front (P, 2) and the reference point (robo_ehvi_eval_cand) -> EHVIResult"""
        front, ref = _ehvi_front(front, ref)
        P = front.shape[0]
        out = np.empty(cand.m) if want_values else None
        trace = np.empty((cand.m, 4)) if (diagnostics and P <= EHVI_MAX_FRONT) else None
        best = _Best()
        check(lib().robo_ehvi_eval_cand(self._h, other._h, cand._h, _arr(front), P, _arr(ref),
                                        _arr(out) if want_values else None, *best.refs,
                                        _arr(trace) if trace is not None else None))
        return EHVIResult(out, *best.values(), trace)

    def cei(self, constraint_gps, cand, thresholds, kind, par, eta, want_values=True, diagnostics=False):
        """constrained expected improvement of ``cand`` with this GP as the objective and ``constraint_gps`` (C of them) as
        the constraints c_k(x) <= thresholds[k]; kind "ei" or "log_ei"; eta None: no feasible incumbent yet, the probability
        of feasibility alone (robo_cei_eval_cand) -> CEIResult"""
        head = self._cei_head(constraint_gps, thresholds, kind, par, eta)
        Cn = head[2]
        out = np.empty(cand.m) if want_values else None
        trace = np.empty((cand.m, 2 * (Cn + 1) + 2)) if (diagnostics and Cn <= CEI_MAX_CONSTRAINTS) else None
        best = _Best()
        check(lib().robo_cei_eval_cand(*head, cand._h, _arr(out) if want_values else None, *best.refs,
                                       _arr(trace) if trace is not None else None))
        return CEIResult(out, *best.values(), trace)

    def _cei_head(self, constraint_gps, thresholds, kind, par, eta):
        """the leading arguments of the fused constrained-EI entry points: (objective, constraints, C, thresholds, kind, par,
        eta, has_eta); the pointer of the thresholds keeps its array alive"""
        constraint_gps = list(constraint_gps)
        Cn = len(constraint_gps)
        return (self._h, _handles(constraint_gps), Cn, _arr(_cei_thresholds(thresholds, Cn)), _cei_kind(kind), float(par),
                0.0 if eta is None else float(eta), int(eta is not None))

    def cei_refine(self, constraint_gps, cand, thresholds, kind, par, eta, n_starts=256, n_steps=50, step0=0.05,
                   diagnostics=False):
        """constrained expected improvement's sweep over ``cand`` (as :meth:`cei`) + multi-start projected gradient ascent on
        the constrained value on the device (robo_cei_refine_cand) -> RefineResult.  The log form ("log_ei") climbs out of
        infeasible regions; in the product form ("ei") a start whose value has underflowed to 0 has no direction and
        freezes.  eta None: the probability of feasibility alone is refined and the objective's GP is only swept."""
        return _refine_call(lib().robo_cei_refine_cand, self._cei_head(constraint_gps, thresholds, kind, par, eta), cand,
                            n_starts, n_steps, step0, diagnostics)

    def sample_paths(self, omega, phase, w, eps):
        """S posterior sample paths of the fitted GP from the caller's draws: omega (F, D) and phase (F,) in the scaled
        space (util/spectral.py draw_features), w (S, F) and eps (S, N) standard normal (robo_paths_create) -> PosteriorPaths"""
        return PosteriorPaths(self, omega, phase, w, eps)


class HyperOptResult(object):
    """robo_gp_optimize_hypers: theta / value / best of the winning start (best -1, NaN: every start was dead); per start
    final (n_starts, P), values, status (0 ran out of iterations, 1 converged, 2 stalled or no direction, 3 dead);
    trace (n_iters + 1, n_starts, 2 P + 3) = [trial theta | F | G | alpha | code] with diagnostics"""

    def __init__(self, theta, value, best, final, values, status, trace=None):
        self.theta, self.value, self.best = theta, value, best
        self.final, self.values, self.status, self.trace = final, values, status, trace


class MESResult(object):
    """values (m,) or None, max, argmax, flags, ystar (K,) the sampled minima ((S, K) in the marginal form); with
    diagnostics: gumbel (7,) / (S, 7) = w_lo, w_hi, w_1/4, w_1/2, w_3/4, a, b and trace (m, 2) / (S, m, 2) the (mean, var)
    the call worked on (include/robo_hip.h)"""

    def __init__(self, values, max, argmax, flags, ystar, gumbel=None, trace=None):
        self.values, self.max, self.argmax, self.flags = values, float(max), int(argmax), int(flags)
        self.ystar, self.gumbel, self.trace = ystar, gumbel, trace


def mes_marginal(gps, eta, cand, u, clamp=True, want_values=True, diagnostics=False, marginal=True):
    """max-value entropy search over device GPs (one: robo_mes_eval_cand; the mean over several hyper-parameter samples,
    each with its own sampled minima: robo_mes_eval_marginal_cand).  eta: one incumbent value, or one per sample;
    u: (K,) or (S, K) uniforms in (0, 1), in the order they are used."""
    S = len(gps)
    u = _f64(u)
    if u.ndim not in (1, 2) or (u.ndim == 2 and u.shape[0] != S) or (u.ndim == 1 and marginal and S != 1):
        raise ValueError("u must be (K,) for one model or (S, K) for %d, got %r" % (S, u.shape))
    K = u.shape[-1]
    ok = 1 <= K <= MES_MAX_K
    shape = (S, K) if marginal else (K,)
    out = np.empty(cand.m) if want_values else None
    ystar = np.full(shape, np.nan)
    gumbel = np.full(shape[:-1] + (7,), np.nan) if diagnostics else None
    trace = np.empty(shape[:-1] + (cand.m, 2)) if (diagnostics and ok) else None
    best = _Best()
    fn = lib().robo_mes_eval_marginal_cand if marginal else lib().robo_mes_eval_cand
    head = _ensemble_head(gps, eta, marginal)
    check(fn(*head, cand._h, _arr(u), K, int(bool(clamp)), _arr(out) if want_values else None, *best.refs, _arr(ystar),
             _arr(gumbel) if diagnostics else None, _arr(trace) if trace is not None else None))
    return MESResult(out, *best.values(), ystar, gumbel, trace)


def mes_sample_min(ctx, mean, var, u, clamp=True, eta=0.0, diagnostics=False):
    """the sampling half of max-value entropy search for (mean, var) of any model over a discretisation
    (robo_mes_sample_min_moments) -> ystar (K,), or (ystar, gumbel (7,)) with diagnostics"""
    mean, var, u = _f64(mean), _f64(var), _f64(u)
    assert mean.ndim == 1 and mean.shape == var.shape and u.ndim == 1
    K = u.shape[0]
    ystar, gumbel = np.full(max(K, 1), np.nan), np.full(7, np.nan)
    check(lib().robo_mes_sample_min_moments(ctx._h, _arr(mean), _arr(var), mean.shape[0], _arr(u), K, int(bool(clamp)),
                                            float(eta), _arr(ystar), _arr(gumbel)))
    return (ystar, gumbel) if diagnostics else ystar


def mes_from_moments(ctx, mean, var, ystar):
    """the element-wise half of max-value entropy search on the device for (mean, var) of any model and given sampled
    minima (robo_mes_eval_moments) -> (values, max, argmax, flags)"""
    mean, var, ystar = _f64(mean), _f64(var), _f64(ystar)
    assert mean.ndim == 1 and mean.shape == var.shape and ystar.ndim == 1
    out = np.empty(mean.shape[0])
    best = _Best()
    check(lib().robo_mes_eval_moments(ctx._h, _arr(mean), _arr(var), mean.shape[0], _arr(ystar), ystar.shape[0], _arr(out),
                                      *best.refs))
    return (out,) + best.values()


class KGResult(object):
    """values (m,) or None, max, argmax, flags, disc_mean (nb,) the posterior mean of the discretisation ((S, nb) in the
    marginal form); with diagnostics: trace (m, nb + 2) / (S, m, nb + 2) = per candidate s_0 .. s_{nb-1}, v, mu(x) as the
    kernel read them (include/robo_hip.h)"""

    def __init__(self, values, max, argmax, flags, disc_mean, trace=None):
        self.values, self.max, self.argmax, self.flags = values, float(max), int(argmax), int(flags)
        self.disc_mean, self.trace = disc_mean, trace


def kg_marginal(gps, cand, rep, sn2s, include_self=True, want_values=True, diagnostics=False, marginal=True):
    """knowledge gradient over device GPs (one: robo_kg_eval_cand; the mean over several hyper-parameter samples, each
    against its own posterior of the shared discretisation ``rep``: robo_kg_eval_marginal_cand).  sn2s: one noise variance
    (in the scale of the returned variances), or one per sample."""
    S = len(gps)
    sn2s = _etas(sn2s, S)
    nb = rep.m
    ok = 1 <= nb <= KG_MAX_DISC
    shape = (S,) if marginal else ()
    out = np.empty(cand.m) if want_values else None
    disc = np.full(shape + (max(nb, 1),), np.nan)
    trace = np.empty(shape + (cand.m, nb + 2)) if (diagnostics and ok) else None
    best = _Best()
    tail = (int(bool(include_self)), _arr(out) if want_values else None) + best.refs + \
        (_arr(disc), _arr(trace) if trace is not None else None)
    if marginal:
        check(lib().robo_kg_eval_marginal_cand(_handles(gps), S, cand._h, rep._h, _arr(sn2s), *tail))
    else:
        check(lib().robo_kg_eval_cand(gps[0]._h, cand._h, rep._h, float(sn2s[0]), *tail))
    return KGResult(out, *best.values(), disc, trace)


def kg_from_moments(ctx, s, v, mean, disc_mean, sn2, include_self=True):
    """the envelope kernel alone on the device for the moments of any model (robo_kg_eval_moments): s (m, nb) signed
    posterior covariances between the candidates and the discretisation, v (m,), mean (m,), disc_mean (nb,)
    -> (values, max, argmax, flags)"""
    s, v, mean, disc_mean = _f64(s), _f64(v), _f64(mean), _f64(disc_mean)
    assert s.ndim == 2 and v.shape == (s.shape[0],) and mean.shape == v.shape and disc_mean.shape == (s.shape[1],)
    out = np.empty(s.shape[0])
    best = _Best()
    check(lib().robo_kg_eval_moments(ctx._h, s.shape[0], s.shape[1], float(sn2), int(bool(include_self)), _arr(s), _arr(v),
                                     _arr(mean), _arr(disc_mean), _arr(out), *best.refs))
    return (out,) + best.values()


class EHVIResult(object):
    """values (m,) or None, max, argmax, flags; with diagnostics: trace (m, 4) = per candidate mean1, var1, mean2, var2 as
    the kernel read them (include/robo_hip.h)"""

    def __init__(self, values, max, argmax, flags, trace=None):
        self.values, self.max, self.argmax, self.flags, self.trace = values, float(max), int(argmax), int(flags), trace


def _ehvi_front(front, ref):
    """(front (P, 2), ref (2,)) contiguous fp64; an empty front in any shape is (0, 2)"""
    front, ref = _f64(front), _f64(ref, (2,))
    if front.size == 0:
        front = np.zeros((0, 2))
    if front.ndim != 2 or front.shape[1] != 2:
        raise ValueError("front must be (P, 2), got %r" % (front.shape,))
    return front, ref


def ehvi_from_moments(ctx, mean1, var1, mean2, var2, front, ref):
    """the strip kernel of the two-objective expected hypervolume improvement alone on the device for the moments of any
    pair of models (robo_ehvi_eval_moments): four (m,) arrays, the sorted front (P, 2), the reference point
    -> (values, max, argmax, flags)"""
    mean1, var1, mean2, var2 = _f64(mean1), _f64(var1), _f64(mean2), _f64(var2)
    assert mean1.ndim == 1 and var1.shape == mean1.shape and mean2.shape == mean1.shape and var2.shape == mean1.shape
    front, ref = _ehvi_front(front, ref)
    out = np.empty(mean1.shape[0])
    best = _Best()
    check(lib().robo_ehvi_eval_moments(ctx._h, mean1.shape[0], _arr(mean1), _arr(var1), _arr(mean2), _arr(var2), _arr(front),
                                       front.shape[0], _arr(ref), _arr(out), *best.refs))
    return (out,) + best.values()


class CEIResult(object):
    """values (m,) or None, max, argmax, flags; with diagnostics: trace (m, 2 (C + 1) + 2) = per candidate the objective's
    (mean, var), every constraint's (mean, var) as the kernel read them, then L = log PoF and the objective factor
    (include/robo_hip.h)"""

    def __init__(self, values, max, argmax, flags, trace=None):
        self.values, self.max, self.argmax, self.flags, self.trace = values, float(max), int(argmax), int(flags), trace


def _cei_kind(kind):
    """the library's number of "ei" / "log_ei"; any other acquisition kind goes through for the library to refuse"""
    return ACQ_KINDS[kind] if kind in ACQ_KINDS else int(kind)


def _cei_thresholds(thresholds, C):
    """(C,) contiguous fp64 (at least one element, so that C = 0 still has an address)"""
    thresholds = _f64(np.asarray(thresholds, dtype=np.float64).reshape(-1))
    if thresholds.shape[0] != C:
        raise ValueError("%d thresholds for %d constraints" % (thresholds.shape[0], C))
    return thresholds if C else np.zeros(1)


def cei_from_moments(ctx, mean0, var0, means, vars, thresholds, kind, par, eta):
    """the fold kernel of constrained expected improvement alone on the device for the moments of any models
    (robo_cei_eval_moments): the objective's mean0, var0 (m,), the constraints' means, vars (C, m), thresholds (C,);
    eta None: no feasible incumbent yet -> (values, max, argmax, flags)"""
    mean0, var0 = _f64(mean0), _f64(var0)
    assert mean0.ndim == 1 and var0.shape == mean0.shape
    m = mean0.shape[0]
    means, vars = _f64(means), _f64(vars)
    assert means.ndim == 2 and means.shape[1] == m and vars.shape == means.shape
    Cn = means.shape[0]
    thresholds = _cei_thresholds(thresholds, Cn)
    out = np.empty(m)
    best = _Best()
    check(lib().robo_cei_eval_moments(ctx._h, m, Cn, _arr(mean0), _arr(var0), _arr(means) if Cn else None,
                                      _arr(vars) if Cn else None, _arr(thresholds), _cei_kind(kind), float(par),
                                      0.0 if eta is None else float(eta), int(eta is not None), _arr(out), *best.refs))
    return (out,) + best.values()


class PathsResult(object):
    """values (S, m) or None, min (S,), argmin (S,) -- per path np.argmax(-f): first index, NaN maximal --, flags"""

    def __init__(self, values, min, argmin, flags):
        self.values, self.min, self.argmin, self.flags = values, min, argmin, int(flags)


class PathsDescentResult(object):
    """x (P, D) the last accepted points in the GP's normalised input space, value (P,), grad (P, D) the gradient there,
    code (P,) the code of the last iteration, flags; with diagnostics: trace (T + 1, P, 2 D + 3) = [trial point, value,
    gradient, step length, 1 accepted / 0 rejected / 2 no trial made / 3 value not finite] per iteration and descent
    (include/robo_hip.h)"""

    def __init__(self, x, value, grad, code, flags, trace=None):
        self.x, self.value, self.grad, self.code, self.flags, self.trace = x, value, grad, code, int(flags), trace


class PathsRefineResult(object):
    """per path: x (S, D) the refined minimiser in the GP's normalised input space, value (S,), start_index (S,) the row of
    the candidate batch the winning descent started from (-1: the path had no start), flags; with diagnostics: starts
    (S, K) rows of all starts in selection order (-1 = slot unused) and trace (T + 1, S K, 2 D + 3) as PathsDescentResult's,
    path-major"""

    def __init__(self, x, value, start_index, flags, starts=None, trace=None):
        self.x, self.value, self.start_index, self.flags = x, value, start_index, int(flags)
        self.starts, self.trace = starts, trace


class PosteriorPaths(object):
    """robo_paths: S posterior sample paths of one fitted GP (Matheron's rule, include/robo_hip.h).  A snapshot: later fits
    of the GP do not change it."""

    def __init__(self, gp, omega, phase, w, eps):
        self._h = None
        omega, phase, w, eps = _f64(omega), _f64(phase), _f64(w), _f64(eps)
        if omega.ndim != 2 or omega.shape[1] != gp.dim:
            raise RoboBadShape("omega must be (F, %d), got %r" % (gp.dim, omega.shape))
        F = omega.shape[0]
        if phase.shape != (F,) or w.ndim != 2 or w.shape[1] != F or eps.shape != (w.shape[0], gp.n):
            raise RoboBadShape("phase must be (F,), w (S, F) and eps (S, N = %d): got %r, %r, %r"
                               % (gp.n, phase.shape, w.shape, eps.shape))
        self.ctx, self.dim, self.n_features, self.n_paths = gp.ctx, gp.dim, F, w.shape[0]
        self._owner = lib()
        h = C.c_void_p()
        check(self._owner.robo_paths_create(gp._h, F, self.n_paths, _arr(omega), _arr(phase), _arr(w), _arr(eps), C.byref(h)))
        self._h = h

    def evaluate(self, Xc, want_values=True):
        """the paths over a Candidates handle or an (m, D) array in the GP's input space -> PathsResult"""
        own = not isinstance(Xc, Candidates)
        cand = Candidates(self.ctx, Xc) if own else Xc
        try:
            S = self.n_paths
            out = np.empty((S, cand.m)) if want_values else None
            mn, am, fl = np.empty(S), np.empty(S, dtype=np.int64), C.c_uint32(0)
            check(lib().robo_paths_eval_cand(self._h, cand._h, _arr(out) if want_values else None, _arr(mn),
                                             am.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(fl)))
            return PathsResult(out, mn, am, fl.value)
        finally:
            if own:
                cand.close()

    def descend(self, path_of, x0, n_steps, step0, diagnostics=False):
        """descent i on path path_of[i] from x0[i] ((P, D) in the GP's normalised input space, inside [0, 1]^D), all in one
        launch (robo_paths_descend) -> PathsDescentResult; n_steps = 0: value and gradient at x0 and nothing else"""
        x0 = _f64(x0)
        if x0.ndim != 2 or x0.shape[1] != self.dim:
            raise RoboBadShape("x0 must be (P, %d), got %r" % (self.dim, x0.shape))
        P, D, T = x0.shape[0], self.dim, int(n_steps)
        path_of = np.ascontiguousarray(path_of, dtype=np.int32)
        if path_of.shape != (P,):
            raise RoboBadShape("path_of must be (%d,), got %r" % (P, path_of.shape))
        want = bool(diagnostics) and 1 <= P <= PATHS_MAX_DESCENTS and T >= 0
        x, val, grad = np.empty((P, D)), np.empty(P), np.empty((P, D))
        code, fl = np.empty(P, dtype=np.int32), C.c_uint32(0)
        trace = np.empty((T + 1, P, 2 * D + 3)) if want else None
        check(lib().robo_paths_descend(self._h, P, path_of.ctypes.data_as(C.POINTER(C.c_int32)), _arr(x0), T, float(step0),
                                       _arr(x), _arr(val), _arr(grad), code.ctypes.data_as(C.POINTER(C.c_int32)),
                                       C.byref(fl), _arr(trace) if want else None))
        return PathsDescentResult(x, val, grad, code, fl.value, trace)

    def refine(self, cand, n_starts, n_steps, step0, diagnostics=False):
        """the sweep over a Candidates handle, per path the n_starts best groups' bests as starts, their descents and the
        winners, without a host round trip (robo_paths_refine_cand) -> PathsRefineResult"""
        S, D, K, T = self.n_paths, self.dim, int(n_starts), int(n_steps)
        want = bool(diagnostics) and 1 <= K <= PATHS_MAX_STARTS and T >= 0
        x, val, si, fl = np.empty((S, D)), np.empty(S), np.empty(S, dtype=np.int64), C.c_uint32(0)
        starts = np.empty((S, K), dtype=np.int64) if want else None
        trace = np.empty((T + 1, S * K, 2 * D + 3)) if want else None
        check(lib().robo_paths_refine_cand(self._h, cand._h, K, T, float(step0), _arr(x), _arr(val),
                                           si.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(fl),
                                           starts.ctypes.data_as(C.POINTER(C.c_int64)) if want else None,
                                           _arr(trace) if want else None))
        return PathsRefineResult(x, val, si, fl.value, starts, trace)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._owner.robo_paths_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchResult(object):
    """indices (q,) rows of the candidate batch in pick order (-1: not made, a NaN winner ended the selection), values (q,),
    fantasies (q, S) the target fantasised after every pick (NaN after the last one made), flags (q,), n_made; with
    diagnostics: trace (q, S, m, 2) the transformed, floored (mean, var) every pick was made from (include/robo_hip.h)"""

    def __init__(self, indices, values, fantasies, flags, n_made, trace=None):
        self.indices, self.values, self.fantasies, self.flags = indices, values, fantasies, flags
        self.n_made, self.trace = int(n_made), trace


def acq_batch(gps, kind, par, eta, cand, q, fantasy="kriging_believer", liar=0.0, diagnostics=False, marginal=True):
    """greedy batch selection over device GPs (one: robo_acq_batch_cand; the mean over several hyper-parameter samples:
    robo_acq_batch_marginal_cand).  eta: one incumbent value, or one per sample.  theta, the constant mean and the output
    transform stay frozen between the picks."""
    if fantasy not in FANTASY_KINDS:
        raise ValueError("fantasy must be one of %s, got %r" % (sorted(FANTASY_KINDS), fantasy))
    S, q = len(gps), int(q)
    ok = 1 <= q <= cand.m
    n = max(q, 1)
    idx = np.full(n, -1, dtype=np.int64)
    val, fant = np.full(n, np.nan), np.full((n, S), np.nan)
    fl = np.zeros(n, dtype=np.uint32)
    made = C.c_int32(0)
    trace = np.empty((q, S, cand.m, 2)) if (diagnostics and ok) else None
    p_idx, p_fl = idx.ctypes.data_as(C.POINTER(C.c_int64)), fl.ctypes.data_as(C.POINTER(C.c_uint32))
    p_trace = _arr(trace) if trace is not None else None
    fn = lib().robo_acq_batch_marginal_cand if marginal else lib().robo_acq_batch_cand
    head = _ensemble_head(gps, eta, marginal, ACQ_KINDS[kind], float(par))
    check(fn(*head, cand._h, q, FANTASY_KINDS[fantasy], float(liar), p_idx, _arr(val), _arr(fant), p_fl, C.byref(made),
             p_trace))
    return BatchResult(idx, val, fant, fl, made.value, trace)


class QEIResult(object):
    """indices (q,) rows of the candidate batch in pick order (-1: not made, a NaN winner ended the selection), gains (q,)
    the winning increments, qei (q,) their running sum (the q-EI estimate of the first j + 1 picks), flags (q,), n_made;
    with diagnostics: acq (q, m), trace (q, S, m, 2), coef (q - 1, S, m), d (q, S), best (q, S, K) (include/robo_hip.h)"""

    def __init__(self, indices, gains, flags, n_made, acq=None, trace=None, coef=None, d=None, best=None):
        self.indices, self.gains, self.flags, self.n_made = indices, gains, flags, int(n_made)
        self.values = gains                         # (what a pick won with: BatchResult's name, for the shared tails)
        self.qei = np.cumsum(gains)
        self.acq, self.trace, self.coef, self.d, self.best = acq, trace, coef, d, best


def qei_batch(gps, par, eta, cand, q, z, diagnostics=False, marginal=True):
    """joint Monte-Carlo batch EI with greedy picks over device GPs (one: robo_qei_batch_cand; the mean over several
    hyper-parameter samples: robo_qei_batch_marginal_cand).  eta: one incumbent value, or one per sample.  z (K, q):
    standard-normal base samples, shared by the samples."""
    S, q = len(gps), int(q)
    z = None if z is None else np.ascontiguousarray(z, dtype=np.float64)
    if z is not None and (z.ndim != 2 or z.shape[1] != max(q, 1)):
        raise ValueError("z must have shape (K, q = %d), got %r" % (q, z.shape))
    K = 0 if z is None else z.shape[0]
    ok = 1 <= q <= cand.m and K >= 1
    n = max(q, 1)
    idx = np.full(n, -1, dtype=np.int64)
    gain = np.full(n, np.nan)
    fl = np.zeros(n, dtype=np.uint32)
    made = C.c_int32(0)
    diag = [None] * 5
    if diagnostics and ok:
        diag = [np.empty((q, cand.m)), np.empty((q, S, cand.m, 2)), np.empty((q - 1, S, cand.m)), np.empty((q, S)),
                np.empty((q, S, K))]
    p_idx, p_fl = idx.ctypes.data_as(C.POINTER(C.c_int64)), fl.ctypes.data_as(C.POINTER(C.c_uint32))
    fn = lib().robo_qei_batch_marginal_cand if marginal else lib().robo_qei_batch_cand
    head = _ensemble_head(gps, eta, marginal, float(par))
    check(fn(*head, cand._h, q, _arr(z) if z is not None else None, K, p_idx, _arr(gain), p_fl, C.byref(made),
             *[_arr(a) if a is not None else None for a in diag]))
    return QEIResult(idx, gain, fl, made.value, *diag)


class RefineResult(object):
    """x (D,) in the GP's normalised input space, value, start_index (row of the candidate batch the winning start came
    from, -1: every candidate was NaN), flags; with diagnostics: starts (K,) rows of all starts in selection order (-1 =
    slot unused) and trace (T + 1, K, 2 D + 3) = [trial point, value, gradient, step length, 1 accepted / 0 rejected /
    2 frozen earlier / 3 variance floored or value not finite at this point] per iteration and start (include/robo_hip.h)"""

    def __init__(self, x, value, start_index, flags, starts=None, trace=None):
        self.x, self.value, self.start_index, self.flags = x, float(value), int(start_index), int(flags)
        self.starts, self.trace = starts, trace


def acq_refine(gps, kind, par, eta, cand, n_starts=256, n_steps=50, step0=0.05, diagnostics=False, marginal=True):
    """the gradient-refined maximiser of a closed-form acquisition over device GPs (one: robo_acq_refine_cand; the mean
    over several hyper-parameter samples: robo_acq_refine_marginal_cand).  eta: one incumbent value, or one per sample."""
    fn = lib().robo_acq_refine_marginal_cand if marginal else lib().robo_acq_refine_cand
    return _refine_call(fn, _ensemble_head(gps, eta, marginal, ACQ_KINDS[kind], float(par)), cand, n_starts, n_steps, step0,
                        diagnostics)


def _refine_call(fn, head, cand, n_starts, n_steps, step0, diagnostics):
    """what the refinement entry points share behind their own leading arguments ``head``: (cand, n_starts, n_steps, step0,
    out_x, out_value, out_start_index, out_flags, out_starts, out_trace) -> RefineResult"""
    K, T, D = int(n_starts), int(n_steps), cand.dim
    x = np.empty(D)
    best = _Best()                           # (value, start index, flags)
    want = bool(diagnostics) and 1 <= K <= REFINE_MAX_STARTS and T >= 0
    starts = np.empty(K, dtype=np.int64) if want else None
    trace = np.empty((T + 1, K, 2 * D + 3)) if want else None
    p_starts = starts.ctypes.data_as(C.POINTER(C.c_int64)) if want else None
    p_trace = _arr(trace) if want else None
    check(fn(*head, cand._h, K, T, float(step0), _arr(x), *best.refs, p_starts, p_trace))
    return RefineResult(x, *best.values(), starts, trace)


def rep_sample_batch(gps, kind, par, etas, lower, upper, normalize, pos, lnp, n_steps, u_stretch, partner, u_accept,
                     a=2.0, diagnostics=False, single=False):
    """S ensemble-sampler chains on the device in one call (robo_rep_sample_batch; ``single``: robo_rep_sample on gps[0]):
    chain s samples exp(acquisition ``kind``) of gps[s] inside the box [lower, upper] of the caller's input space.
    pos (S, k, D) start positions; lnp (S, k) their log-probabilities or None = evaluate them; draws (S, n_steps, 2, k / 2).
    -> (pos, lnp, accepted (S, k) int64, flags (S,) uint32, trace (S, n_steps, 2, k / 2, D + 2) or None); a trace row is
    (q, lnp(q), code 0 rejected / 1 accepted / 2 outside the box)."""
    S = len(gps)
    pos = np.array(pos, dtype=np.float64, order="C")
    assert pos.ndim == 3 and pos.shape[0] == S
    k, D = pos.shape[1], pos.shape[2]
    T, half = int(n_steps), k // 2
    eval_start = lnp is None
    lnp = np.zeros((S, k)) if eval_start else np.array(lnp, dtype=np.float64, order="C").reshape(S, k)
    uz = np.ascontiguousarray(u_stretch, dtype=np.float64).reshape(-1)
    ua = np.ascontiguousarray(u_accept, dtype=np.float64).reshape(-1)
    pa = np.ascontiguousarray(partner, dtype=np.int32).reshape(-1)
    assert uz.size == ua.size == pa.size == S * T * 2 * half
    lower, upper = _f64(lower, (D,)), _f64(upper, (D,))
    acc = np.zeros((S, k), dtype=np.int64)
    flags = np.zeros(S, dtype=np.uint32)
    trace = np.empty((S, T, 2, half, D + 2)) if diagnostics else None
    tail = (_arr(lower), _arr(upper), int(bool(normalize)), k, T, float(a), _arr(uz), pa.ctypes.data_as(C.POINTER(C.c_int32)),
            _arr(ua), _arr(pos), _arr(lnp), int(eval_start), acc.ctypes.data_as(C.POINTER(C.c_int64)),
            flags.ctypes.data_as(C.POINTER(C.c_uint32)), _arr(trace) if diagnostics else None)
    fn = lib().robo_rep_sample if single else lib().robo_rep_sample_batch
    check(fn(*_ensemble_head(gps, etas, not single, ACQ_KINDS[kind], float(par)), *tail))
    return pos, lnp, acc, flags, trace


def rep_sample(gp, kind, par, eta, lower, upper, normalize, pos, lnp, n_steps, u_stretch, partner, u_accept, a=2.0,
               diagnostics=False):
    """one chain (robo_rep_sample): the arrays of :func:`rep_sample_batch` without the leading S axis"""
    pos = np.asarray(pos, dtype=np.float64)
    res = rep_sample_batch([gp], kind, par, eta, lower, upper, normalize, pos[None], None if lnp is None else
                           np.asarray(lnp, dtype=np.float64)[None], n_steps, u_stretch, partner, u_accept, a, diagnostics,
                           single=True)
    return tuple(None if r is None else r[0] for r in res)


class Comm(object):
    """robo_comm: this process's rank in a one-process-per-GPU job; the exchanges of the candidate / sample shards run
    inside the library as RCCL all-gathers on the context's stream (include/robo_hip.h).  Every method is COLLECTIVE."""

    @staticmethod
    def create_id():
        """rank 0: the 128-byte id every rank must be given (out of band) before constructing its Comm"""
        buf = C.create_string_buffer(COMM_ID_BYTES)
        check(lib().robo_comm_create_id(buf))
        return bytes(buf.raw)

    def __init__(self, ctx, rank, world, comm_id):
        assert len(comm_id) == COMM_ID_BYTES
        self.ctx, self.rank, self.world = ctx, int(rank), int(world)
        self._h = C.c_void_p()
        self._owner = lib()
        check(self._owner.robo_comm_init(ctx._h, self.rank, self.world, bytes(comm_id), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._owner.robo_comm_destroy(self._h)
            self._h = None

    def info(self):
        """(rank, world) as the communicator holds them (robo_comm_info)"""
        r, w = C.c_int32(-1), C.c_int32(-1)
        check(lib().robo_comm_info(self._h, C.byref(r), C.byref(w)))
        return int(r.value), int(w.value)

    def allgather(self, values):
        """values: (count,) host doubles -> (world, count), identical on every rank"""
        v = _f64(np.asarray(values, dtype=np.float64).reshape(-1))
        out = np.empty((self.world, v.shape[0]))
        check(lib().robo_comm_allgather(self._h, _arr(v), v.shape[0], _arr(out)))
        return out

    def acq_sharded(self, gp, kind, par, eta, cand, global_offset, want_values=False):
        """candidate shard -> (this rank's values or None, GLOBAL max, GLOBAL argmax, owner rank, flags OR-ed)"""
        out = np.empty(cand.m) if want_values else None
        mx, am, own, fl = C.c_double(0), C.c_int64(0), C.c_int32(0), C.c_uint32(0)
        check(lib().robo_acq_eval_cand_sharded(self._h, gp._h, ACQ_KINDS[kind], float(par), float(eta), cand._h,
                                               int(global_offset), _arr(out) if want_values else None, C.byref(mx),
                                               C.byref(am), C.byref(own), C.byref(fl)))
        return out, mx.value, am.value, own.value, fl.value

    def ig_per_cost_sharded(self, gp, cand, rep, ep, sn2, cost_gp, cost_cand, overhead, global_offset,
                            want_values=False):
        """candidate shard of the information gain per unit cost -> (this rank's values or None, GLOBAL max, GLOBAL
        argmax, owner rank)"""
        assert rep.m == ep.nb and cost_cand.m == cand.m
        out = np.empty(cand.m) if want_values else None
        mx, am, own = C.c_double(0), C.c_int64(0), C.c_int32(0)
        check(lib().robo_ig_eval_per_cost_cand_sharded(self._h, gp._h, cand._h, rep._h, ep.W.size, float(sn2),
                                                       *ep.args(), cost_gp._h, cost_cand._h, float(overhead),
                                                       int(global_offset), _arr(out) if want_values else None,
                                                       C.byref(mx), C.byref(am), C.byref(own)))
        return out, mx.value, am.value, own.value

    def acq_marginal_sharded(self, gps, s_total, kind, par, etas, cand, want_values=True):
        """sample shard: this rank's fitted GPs (possibly none) -> (mean over ALL s_total samples or None, max,
        argmax, flags), identical on every rank"""
        S = len(gps)
        etas = _f64(np.asarray(etas, dtype=np.float64).reshape(-1)) if S else np.zeros(1)
        out = np.empty(cand.m) if want_values else None
        best = _Best()
        check(lib().robo_acq_eval_marginal_cand_sharded(self._h, _handles(gps), S, int(s_total), ACQ_KINDS[kind], float(par),
                                                        _arr(etas), cand._h, _arr(out) if want_values else None,
                                                        *best.refs))
        return (out,) + best.values()


class CandidateShards(object):
    """the candidate batch of ONE maximisation split over the contexts of a Multi: shards[g] is a Candidates on context g
    (or None: empty shard), offsets[g] the global index of its first row"""

    def __init__(self, shards, offsets):
        self.shards, self.offsets = list(shards), [int(o) for o in offsets]
        self.m = sum(c.m for c in self.shards if c is not None)

    @classmethod
    def split(cls, ctxs, Xn):
        """contiguous shards of the host matrix Xn (already in the model's input space), one upload per device"""
        Xn = _f64(Xn)
        shards, offsets = [], []
        for g, ctx in enumerate(ctxs):
            b, e = shard_range(Xn.shape[0], g, len(ctxs))
            offsets.append(b)
            shards.append(Candidates(ctx, Xn[b:e]) if e > b else None)
        return cls(shards, offsets)

    def owner_point(self, owner, global_index):
        return self.shards[owner].point(int(global_index) - self.offsets[owner])

    def point(self, global_index):
        """row `global_index` of the whole batch, from whichever shard holds it"""
        for g, c in enumerate(self.shards):
            if c is not None and self.offsets[g] <= global_index < self.offsets[g] + c.m:
                return self.owner_point(g, global_index)
        raise IndexError(global_index)

    def close(self):
        for c in self.shards:
            if c is not None:
                c.close()


class Multi(object):
    """robo_multi: G contexts of THIS process, one per device; every method fans its shards out to all devices at once
    (one worker thread per device inside the library) and returns the reduced result (include/robo_hip.h)."""

    def __init__(self, ctxs):
        self.ctxs = list(ctxs)
        self.n = len(self.ctxs)
        arr = (C.c_void_p * self.n)(*[c._h for c in self.ctxs])
        self._h = C.c_void_p()
        self._lib = lib()            # the library that owns the handle (tests switch libraries: use_library)
        check(self._lib.robo_multi_create(arr, self.n, C.byref(self._h)))
        _live_multis.add(self)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.robo_multi_destroy(self._h)      # joins the worker threads
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """(number of contexts, their HIP devices, worker threads in use)"""
        n, t = C.c_int32(0), C.c_int32(0)
        dev = (C.c_int32 * self.n)()
        check(lib().robo_multi_info(self._h, C.byref(n), dev, C.byref(t)))
        return int(n.value), [int(d) for d in dev], int(t.value)

    def _handles(self, objs):
        return (C.c_void_p * max(len(objs), 1))(*[(o._h if o is not None else None) for o in objs])

    @staticmethod
    def _flatten(groups):
        flat = [g for grp in groups for g in grp]
        counts = (C.c_int32 * len(groups))(*[len(grp) for grp in groups])
        return flat, counts

    def set_data(self, gps, X, y):
        X, y = _f64(X), _f64(y)
        assert len(gps) == self.n and X.ndim == 2 and y.shape == (X.shape[0],)
        check(lib().robo_gp_set_data_multi(self._h, self._handles(gps), _arr(X), _arr(y), X.shape[0]))
        for g in gps:
            g.n = X.shape[0]

    def fit(self, gps, theta, mean_c):
        """the same fit on every device's replica -> log-likelihood; raises np.linalg.LinAlgError like DeviceGP.fit"""
        assert len(gps) == self.n
        theta = _f64(_full_theta(gps[0], theta), (gps[0].n_theta,))
        ll, col = C.c_double(0), C.c_int32(0)
        check(lib().robo_gp_fit_multi(self._h, self._handles(gps), _arr(theta), float(mean_c), C.byref(ll), C.byref(col)))
        return ll.value

    def loglik_batch(self, gps, thetas, mean_c):
        """DeviceGP.loglik_batch with the thetas split over the devices (gps: one data-holding handle per device)"""
        assert len(gps) == self.n
        thetas = _f64(_full_theta(gps[0], np.atleast_2d(thetas)))
        S = thetas.shape[0]
        ll = np.empty(S)
        st = np.empty(S, dtype=np.int32)
        check(lib().robo_gp_loglik_batch_multi(self._h, self._handles(gps), _arr(thetas), S, float(mean_c), _arr(ll),
                                               st.ctypes.data_as(C.POINTER(C.c_int32))))
        return ll, st

    def fit_batch(self, gp_groups, thetas, mean_c):
        """fit_batch per device: gp_groups[g] = the handles of device g (its first one holds the data), thetas in the
        flattened order -> (loglik, status)"""
        assert len(gp_groups) == self.n
        flat, counts = self._flatten(gp_groups)
        thetas = _f64(_full_theta(flat[0], np.atleast_2d(thetas))) if flat else _f64(thetas)
        assert thetas.shape[0] == len(flat)
        ll = np.empty(len(flat))
        st = np.empty(len(flat), dtype=np.int32)
        check(lib().robo_gp_fit_batch_multi(self._h, self._handles(flat), counts, _arr(thetas), float(mean_c), _arr(ll),
                                            st.ctypes.data_as(C.POINTER(C.c_int32))))
        n = next((grp[0].n for grp in gp_groups if grp), 0)
        for g in flat:
            g.n = n
        return ll, st

    def acq(self, gps, kind, par, eta, shards, want_values=False):
        """candidate shard -> (values of all shards in slot order or None, max, GLOBAL argmax, owner slot, flags OR-ed)"""
        assert len(gps) == self.n and len(shards.shards) == self.n
        out = np.empty(shards.m) if want_values else None
        mx, am, own, fl = C.c_double(0), C.c_int64(0), C.c_int32(0), C.c_uint32(0)
        offs = (C.c_int64 * self.n)(*shards.offsets)
        check(lib().robo_acq_eval_cand_multi(self._h, self._handles(gps), ACQ_KINDS[kind], float(par), float(eta),
                                             self._handles(shards.shards), offs, _arr(out) if want_values else None,
                                             C.byref(mx), C.byref(am), C.byref(own), C.byref(fl)))
        return out, mx.value, am.value, own.value, fl.value

    def ig(self, gps, shards, reps, ep, sn2, want_values=True):
        """candidate shard of the information gain -> (values of all shards in slot order or None, max, GLOBAL argmax, owner)"""
        assert all(len(x) == self.n for x in (gps, shards.shards, reps))
        out = np.empty(shards.m) if want_values else None
        mx, am, own = C.c_double(0), C.c_int64(0), C.c_int32(0)
        offs = (C.c_int64 * self.n)(*shards.offsets)
        check(lib().robo_ig_eval_cand_multi(self._h, self._handles(gps), self._handles(shards.shards), self._handles(reps),
                                            ep.W.size, float(sn2), *ep.args(), offs, _arr(out) if want_values else None,
                                            C.byref(mx), C.byref(am), C.byref(own)))
        return out, mx.value, am.value, own.value

    def ig_per_cost(self, gps, shards, reps, ep, sn2, cost_gps, cost_shards, overhead, want_values=False):
        """candidate shard of the information gain per unit cost -> (values or None, max, GLOBAL argmax, owner slot)"""
        assert all(len(x) == self.n for x in (gps, shards.shards, reps, cost_gps, cost_shards.shards))
        out = np.empty(shards.m) if want_values else None
        mx, am, own = C.c_double(0), C.c_int64(0), C.c_int32(0)
        offs = (C.c_int64 * self.n)(*shards.offsets)
        check(lib().robo_ig_eval_per_cost_cand_multi(self._h, self._handles(gps), self._handles(shards.shards),
                                                     self._handles(reps), ep.W.size, float(sn2), *ep.args(),
                                                     self._handles(cost_gps), self._handles(cost_shards.shards),
                                                     float(overhead), offs, _arr(out) if want_values else None,
                                                     C.byref(mx), C.byref(am), C.byref(own)))
        return out, mx.value, am.value, own.value

    def acq_marginal(self, gp_groups, kind, par, eta_groups, cands, want_values=True):
        """sample shard: gp_groups[g] / eta_groups[g] = the fitted handles of device g and their incumbent values,
        cands[g] = ALL candidates on device g (None where a device has no sample, g > 0) -> (mean over all samples or
        None, max, argmax, flags)"""
        assert len(gp_groups) == self.n and len(cands) == self.n
        flat, counts = self._flatten(gp_groups)
        etas = _f64(np.concatenate([np.asarray(e, dtype=np.float64).reshape(-1) for e in eta_groups] or [np.zeros(0)]))
        assert etas.shape[0] == len(flat)
        out = np.empty(cands[0].m) if want_values else None
        best = _Best()
        check(lib().robo_acq_eval_marginal_cand_multi(self._h, self._handles(flat), counts, ACQ_KINDS[kind], float(par),
                                                      _arr(etas), self._handles(cands),
                                                      _arr(out) if want_values else None, *best.refs))
        return (out,) + best.values()

    def predict_mixture(self, gp_groups, cands):
        """GaussianProcessMCMC.predict over samples that live on several devices -> (mean (M,), var (M,))"""
        assert len(gp_groups) == self.n and len(cands) == self.n
        flat, counts = self._flatten(gp_groups)
        mean, var = np.empty(cands[0].m), np.empty(cands[0].m)
        check(lib().robo_gp_predict_mixture_cand_multi(self._h, self._handles(flat), counts, self._handles(cands),
                                                       _arr(mean), _arr(var)))
        return mean, var


def fit_batch(gps, thetas, mean_c):
    """GaussianProcessMCMC.train's per-sample fits in one batched pass that keeps the factors:
    gps[0] holds the data; afterwards gps[s] is fitted at thetas[s] wherever status[s] == OK.
    -> (loglik (S,), status (S,))"""
    S = len(gps)
    thetas = _f64(_full_theta(gps[0], np.atleast_2d(thetas)))
    assert thetas.shape == (S, gps[0].n_theta)
    ll = np.empty(S)
    st = np.empty(S, dtype=np.int32)
    check(lib().robo_gp_fit_batch(_handles(gps), S, _arr(thetas), float(mean_c), _arr(ll), st.ctypes.data_as(C.POINTER(C.c_int32))))
    for g in gps:
        g.n = gps[0].n
    return ll, st


def predict_mixture(gps, cand):
    """GaussianProcessMCMC.predict over device GPs -> (mean (M,), var (M,))"""
    S = len(gps)
    mean, var = np.empty(cand.m), np.empty(cand.m)
    check(lib().robo_gp_predict_mixture_cand(_handles(gps), S, cand._h, _arr(mean), _arr(var)))
    return mean, var


def acq_from_moments(ctx, kind, par, eta, mean, var):
    """element-wise acquisition on the device for (mean, var) of any model -> (values, max, argmax, flags)"""
    mean, var = _f64(mean), _f64(var)
    assert mean.ndim == 1 and mean.shape == var.shape
    out = np.empty(mean.shape[0])
    best = _Best()
    check(lib().robo_acq_eval_moments(ctx._h, ACQ_KINDS[kind], float(par), float(eta), _arr(mean), _arr(var),
                                      mean.shape[0], _arr(out), *best.refs))
    return (out,) + best.values()


class EPState(object):
    """the host-side EP tensors of entropy search, contiguous fp64"""

    def __init__(self, logP, lmb, W, dlogPdMu, dlogPdSigma, dlogPdMudMu):
        self.nb = int(np.asarray(logP).size)
        self.logP = _f64(np.asarray(logP).reshape(-1))
        self.lmb = _f64(np.asarray(lmb).reshape(-1))
        self.W = _f64(np.asarray(W).reshape(-1))
        self.dMu = _f64(dlogPdMu, (self.nb, self.nb))
        self.dSigma = _f64(dlogPdSigma, (self.nb, self.nb * (self.nb + 1) // 2))
        self.dMuMu = _f64(dlogPdMudMu, (self.nb, self.nb, self.nb))

    def args(self):
        return [_arr(a) for a in (self.logP, self.lmb, self.W, self.dMu, self.dSigma, self.dMuMu)]


def ig_eval(gp, cand, rep, ep, sn2, want_values=True):
    """information gain of every candidate -> (values, max, argmax)"""
    assert rep.m == ep.nb
    out = np.empty(cand.m) if want_values else None
    mx, am = C.c_double(0), C.c_int64(0)
    check(lib().robo_ig_eval_cand(gp._h, cand._h, rep._h, ep.W.size, float(sn2), *ep.args(),
                                  _arr(out) if want_values else None, C.byref(mx), C.byref(am)))
    return out, mx.value, am.value


def ig_eval_per_cost(gp, cand, rep, ep, sn2, cost_gp, cost_cand, overhead=0.0, want_values=True):
    """information gain per unit cost of every candidate, dH / (exp(cost mean) + overhead), and its argmax, in one
    library call -> (values or None, max, argmax)"""
    assert rep.m == ep.nb and cost_cand.m == cand.m
    out = np.empty(cand.m) if want_values else None
    mx, am = C.c_double(0), C.c_int64(0)
    check(lib().robo_ig_eval_per_cost_cand(gp._h, cand._h, rep._h, ep.W.size, float(sn2), *ep.args(), cost_gp._h,
                                           cost_cand._h, float(overhead), _arr(out) if want_values else None,
                                           C.byref(mx), C.byref(am)))
    return out, mx.value, am.value


def ig_from_moments(ctx, s, v, ep, sn2):
    s, v = _f64(s), _f64(v)
    assert s.ndim == 2 and s.shape[1] == ep.nb and v.shape == (s.shape[0],)
    out = np.empty(s.shape[0])
    check(lib().robo_ig_eval_moments(ctx._h, s.shape[0], ep.nb, ep.W.size, float(sn2), _arr(s), _arr(v), *ep.args(),
                                     _arr(out)))
    return out


def ep_joint_min(ctx, mu, sigma, with_derivatives=False):
    """EP p_min of S beliefs on the device (robo_ep_joint_min): mu (S, N), sigma (S, N, N) ->
    (logP (S, N), dlogPdMu (S, N, N), dlogPdSigma (S, N, N(N+1)/2), dlogPdMudMu (S, N, N, N), sweeps (S, N)), the three
    derivatives None without ``with_derivatives``; sweeps[s, k] = EP sweeps of minimiser k, -1 where it was killed.
    The first belief whose status is not OK raises what epmgp.joint_min raises on it (LinAlgError / Exception)."""
    mu = _f64(mu)
    if mu.ndim != 2:
        raise AssertionError("mu must be (S, N), got %r" % (mu.shape,))
    S, n = mu.shape
    sigma = _f64(sigma, (S, n, n))
    i32p = C.POINTER(C.c_int32)
    logP = np.empty((S, n))
    d = (np.empty((S, n, n)), np.empty((S, n, n * (n + 1) // 2)), np.empty((S, n, n, n))) if with_derivatives else None
    sweeps = np.empty((S, n), dtype=np.int32)
    status = np.empty(S, dtype=np.int32)
    check(lib().robo_ep_joint_min(ctx._h, int(S), int(n), _arr(mu), _arr(sigma), 1 if with_derivatives else 0,
                                  _arr(logP), *([_arr(a) for a in d] if d else [None, None, None]),
                                  sweeps.ctypes.data_as(i32p), status.ctypes.data_as(i32p)))
    for st in status:
        if st == NOT_POSITIVE_DEFINITE:
            raise np.linalg.LinAlgError("Matrix is not positive definite")
        check(int(st), msg="robo_ep_joint_min: belief status %d" % st)
    if d is None:
        return logP, None, None, None, sweeps
    return (logP,) + d + (sweeps,)


def pmin_mc(ctx, mu, sigma, z):
    """Monte-Carlo p_min of S beliefs on the device with the given draws (robo_pmin_mc): mu (S, N), sigma (S, N, N),
    z (Nf, N) standard normals -> (pmin (S, N), jitter (S,)).  A belief without a factor (jitter beyond 1e4) raises
    np.linalg.LinAlgError, as mc_part.joint_pmin does."""
    mu = _f64(mu)
    if mu.ndim != 2:
        raise AssertionError("mu must be (S, N), got %r" % (mu.shape,))
    S, n = mu.shape
    sigma = _f64(sigma, (S, n, n))
    z = _f64(z)
    if z.ndim != 2 or z.shape[1] != n:
        raise AssertionError("z must be (Nf, %d), got %r" % (n, z.shape))
    pmin, jitter = np.empty((S, n)), np.empty(S)
    status = np.empty(S, dtype=np.int32)
    check(lib().robo_pmin_mc(ctx._h, int(S), int(n), int(z.shape[0]), _arr(mu), _arr(sigma), _arr(z), _arr(pmin),
                             _arr(jitter), status.ctypes.data_as(C.POINTER(C.c_int32))))
    for st in status:
        if st == NOT_POSITIVE_DEFINITE:
            raise np.linalg.LinAlgError("Cholesky decomposition failed.")
        check(int(st), msg="robo_pmin_mc: belief status %d" % st)
    return pmin, jitter


class MCState(object):
    """the per-update state of InformationGainMC, contiguous fp64: the draws z (Nf, Nb), the belief Mb (Nb), Vb (Nb, Nb)
    at the representer points, logP (Nb) = log of its p_min, lmb (Nb) and the outcome quantiles W (Np).  The library
    uploads z once and reuses it while the same draws come back (every compute() of an update)."""

    def __init__(self, z, Mb, Vb, logP, lmb, W):
        self.z = _f64(z)
        self.nf, self.nb = self.z.shape
        self.Mb = _f64(np.asarray(Mb).reshape(-1))
        self.Vb = _f64(Vb, (self.nb, self.nb))
        self.logP = _f64(np.asarray(logP).reshape(-1))
        self.lmb = _f64(np.asarray(lmb).reshape(-1))
        self.W = _f64(np.asarray(W).reshape(-1))
        assert self.Mb.size == self.logP.size == self.lmb.size == self.nb

    def args(self):
        return [_arr(a) for a in (self.Mb, self.Vb, self.logP, self.lmb, self.W, self.z)]


def igmc_eval(gp, cand, rep, mc, sn2, want_values=True):
    """Monte-Carlo information gain of every candidate (robo_igmc_eval_cand) -> (values or None, max, argmax, flags)"""
    assert rep.m == mc.nb
    out = np.empty(cand.m) if want_values else None
    best = _Best()
    check(lib().robo_igmc_eval_cand(gp._h, cand._h, rep._h, mc.W.size, mc.nf, float(sn2), *mc.args(),
                                    _arr(out) if want_values else None, *best.refs))
    return (out,) + best.values()


def igmc_from_moments(ctx, s, v, mc, sn2, with_counts=False):
    """the same from s (m, Nb) and v (m,) of any model (robo_igmc_eval_moments) -> values, or (values, counts
    (m, Np, Nb) int32, jitter (m,)) with ``with_counts``"""
    s, v = _f64(s), _f64(v)
    assert s.ndim == 2 and s.shape[1] == mc.nb and v.shape == (s.shape[0],)
    m = s.shape[0]
    out = np.empty(m)
    counts = np.empty((m, mc.W.size, mc.nb), dtype=np.int32) if with_counts else None
    jitter = np.empty(m) if with_counts else None
    check(lib().robo_igmc_eval_moments(ctx._h, m, mc.nb, mc.W.size, mc.nf, float(sn2), _arr(s), _arr(v), *mc.args(),
                                       _arr(out), counts.ctypes.data_as(C.POINTER(C.c_int32)) if with_counts else None,
                                       _arr(jitter) if with_counts else None))
    return (out, counts, jitter) if with_counts else out


def cross_cov(gp, cand, ref):
    out = np.empty((cand.m, ref.m))
    check(lib().robo_gp_cross_cov(gp._h, cand._h, ref._h, _arr(out)))
    return out


def acq_marginal(gps, kind, par, eta, cand, want_values=True, reduce="mean"):
    """MarginalizationGPMCMC.compute over device GPs -> (values, max, argmax, flags).
    eta: one incumbent value for all samples, or one per sample (S,)."""
    S = len(gps)
    arr, etas = _handles(gps), _etas(eta, S)
    best = _Best()
    out = np.empty(cand.m) if (want_values or reduce == "sum") else None
    if reduce == "sum":
        check(lib().robo_acq_eval_sum_cand(arr, S, ACQ_KINDS[kind], float(par), _arr(etas), cand._h, _arr(out),
                                           best.refs[2]))
        return out, None, None, best.flags.value
    check(lib().robo_acq_eval_marginal_cand(arr, S, ACQ_KINDS[kind], float(par), _arr(etas), cand._h,
                                            _arr(out) if want_values else None, *best.refs))
    return (out,) + best.values()
