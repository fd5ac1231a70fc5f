// C ABI of librobo_hip.so, part 6: the two-objective expected hypervolume improvement (robo_ehvi_eval_cand,
// robo_ehvi_eval_moments; the rule is stated in include/robo_hip.h).  Host-side orchestration only: every number is
// produced by the kernels in predict.hip / ehvi.hip / acq.hip.
#include <cmath>

#include "api_internal.h"

namespace robo {
constexpr const char* EHVI_LABEL = "expected hypervolume improvement";

// the front as the rule needs it: 0 <= P <= ROBO_EHVI_MAX_FRONT finite points, a strictly ascending, b strictly
// descending, every point strictly below the finite reference point
static int ehvi_check(const double* front, int64_t P, const double* ref) {
    if (!ref || P < 0 || P > ROBO_EHVI_MAX_FRONT || (P > 0 && !front)) {
        set_error("%s: a front of %lld points, must be in [0, %d], with a reference point", EHVI_LABEL, (long long)P,
                  ROBO_EHVI_MAX_FRONT);
        return ROBO_BAD_ARGUMENT;
    }
    if (!std::isfinite(ref[0]) || !std::isfinite(ref[1])) {
        set_error("%s: the reference point (%g, %g) is not finite", EHVI_LABEL, ref[0], ref[1]);
        return ROBO_BAD_ARGUMENT;
    }
    for (int64_t i = 0; i < P; ++i) {
        const double a = front[2 * i], b = front[2 * i + 1];
        if (!std::isfinite(a) || !std::isfinite(b) || !(a < ref[0]) || !(b < ref[1])) {
            set_error("%s: front point %lld = (%g, %g) is not finite and strictly below the reference point (%g, %g)",
                      EHVI_LABEL, (long long)i, a, b, ref[0], ref[1]);
            return ROBO_BAD_ARGUMENT;
        }
        if (i > 0 && !(front[2 * i - 2] < a && front[2 * i - 1] > b)) {
            set_error("%s: the front must be sorted with its first objective strictly ascending and its second strictly "
                      "descending (points %lld and %lld)", EHVI_LABEL, (long long)i - 1, (long long)i);
            return ROBO_BAD_ARGUMENT;
        }
    }
    return ROBO_OK;
}

// [front (ROBO_EHVI_MAX_FRONT x 2) | trace (m x 4)] on the handle (the diagnostics buffer the knowledge gradient uses),
// the front uploaded (asynchronous: the caller's array outlives the call's synchronisation)
static int ehvi_stage_front(robo_cand* k, const double* front, int P, size_t trace_len) {
    ROBO_TRY(dev_grow(k->ctx->stream, &k->d_kg, &k->kg_cap, (size_t)2 * ROBO_EHVI_MAX_FRONT + trace_len));
    if (P > 0)
        ROBO_HIP_CHECK(hipMemcpyAsync(k->d_kg, front, (size_t)2 * P * sizeof(double), hipMemcpyHostToDevice, k->ctx->stream));
    return ROBO_OK;
}

}  // namespace robo

using namespace robo;

extern "C" {

int32_t robo_ehvi_eval_cand(robo_gp* gp1, robo_gp* gp2, robo_cand* k, const double* front, int32_t P, const double* ref,
                            double* out_ehvi, double* out_max, int64_t* out_argmax, uint32_t* out_flags, double* out_trace) {
    if (!gp1 || !gp2 || !k) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(ehvi_check(front, P, ref));
    if (gp1->ctx != gp2->ctx || k->ctx != gp1->ctx) {
        set_error("%s: the two GPs and the candidates must live on one context", EHVI_LABEL);
        return ROBO_BAD_ARGUMENT;
    }
    if (gp1->dim != k->dim || gp2->dim != k->dim) {
        set_error("%s: the GPs (dim %d, %d) do not match the candidates (dim %d)", EHVI_LABEL, gp1->dim, gp2->dim, k->dim);
        return ROBO_BAD_SHAPE;
    }
    if (!gp1->fitted || !gp2->fitted) {
        set_error("Model has to be trained first!");
        return ROBO_NOT_FITTED;
    }
    robo_ctx* c = k->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    const size_t trace_len = out_trace ? (size_t)k->m * 4 : 0;
    ROBO_TRY(ehvi_stage_front(k, front, P, trace_len));
    // the two sweeps, each chunked by the workspace: rows 0 and 1 of the handle's sample tables
    robo_gp* gps[2] = {gp1, gp2};
    ROBO_TRY(clear_flags_on_error(k, predict_samples(gps, 2, k, 2)));
    double* d_trace = out_trace ? k->d_kg + (size_t)2 * ROBO_EHVI_MAX_FRONT : nullptr;
    // event slots 30 -> 31 bracket the strip kernel, under the condition of slots 24..27
    const bool ev = c->phase_events || k->m_pad > 16384;
    if (ev) ROBO_HIP_CHECK(hipEventRecord(c->events[30], c->stream));
    ROBO_TRY(clear_flags_on_error(k, launch_ehvi(c, k->d_mu_all, k->d_var_all, k->d_mu_all + k->m_pad, k->d_var_all + k->m_pad,
                                                 k->d_kg, P, ref[0], ref[1], k->m, k->d_acq_sum, k->d_flags, d_trace)));
    if (ev) ROBO_HIP_CHECK(hipEventRecord(c->events[31], c->stream));
    ROBO_TRY(clear_flags_on_error(k, launch_argmax(k, k->d_acq_sum, 1.0)));
    ROBO_TRY(finish_call(k, EHVI_LABEL, ROBO_OK, {{out_trace, d_trace, trace_len * sizeof(double)}}, false));
    // (max, argmax, flags) [+ the values] and the one synchronisation of the call
    return clear_flags_on_error(k, acq_read_back(k, k->d_acq, out_ehvi, out_max, out_argmax, out_flags));
}

int32_t robo_ehvi_eval_moments(robo_ctx* ctx, int64_t m, const double* mean1, const double* var1, const double* mean2,
                               const double* var2, const double* front, int32_t P, const double* ref, double* out_ehvi,
                               double* out_max, int64_t* out_argmax, uint32_t* out_flags) {
    if (!ctx || !mean1 || !var1 || !mean2 || !var2) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(ehvi_check(front, P, ref));
    robo_cand* k = nullptr;
    ROBO_TRY(moments_handle(ctx, mean1, var1, m, "expected hypervolume improvement: upload of the moments", &k));
    // the second objective's moments ride in the handle's d_mu / d_q (m_pad doubles each, otherwise unused here)
    int st = ehvi_stage_front(k, front, P, 0);
    if (st == ROBO_OK) {
        hipError_t e = hipMemcpyAsync(k->d_mu, mean2, (size_t)m * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(k->d_q, var2, (size_t)m * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) {
            set_error("%s: upload of the moments failed: %s", EHVI_LABEL, hipGetErrorString(e));
            st = ROBO_RUNTIME_ERROR;
        }
    }
    if (st == ROBO_OK)
        st = launch_ehvi(ctx, k->d_mean, k->d_var, k->d_mu, k->d_q, k->d_kg, P, ref[0], ref[1], m, k->d_acq_sum, k->d_flags,
                         nullptr);
    if (st == ROBO_OK) st = launch_argmax(k, k->d_acq_sum, 1.0);
    if (st == ROBO_OK) st = acq_read_back(k, k->d_acq, out_ehvi, out_max, out_argmax, out_flags);
    else hipStreamSynchronize(ctx->stream);
    robo_cand_destroy(k);
    return st;
}

}  // extern "C"
