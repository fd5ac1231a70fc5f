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
    robo_gp* gps[2] = {gp1, gp2};
    ROBO_TRY(models_check(EHVI_LABEL, "the two GPs", gps, 2, k, [&](int) {
        set_error("%s: the GPs (dim %d, %d) do not match the candidates (dim %d)", EHVI_LABEL, gp1->dim, gp2->dim, k->dim);
    }));
    const size_t trace_len = out_trace ? (size_t)k->m * 4 : 0;
    ROBO_TRY(ehvi_stage_front(k, front, P, trace_len));
    double* d_trace = out_trace ? k->d_kg + (size_t)2 * ROBO_EHVI_MAX_FRONT : nullptr;
    // the two objectives' posteriors are rows 0 and 1 of the handle's sample tables; slots 30 -> 31 bracket the strip kernel
    return models_fold(EHVI_LABEL, gps, 2, k, EV_FOLD_BEGIN, [&] {
        return launch_ehvi(k->ctx, k->d_mu_all, k->d_var_all, k->d_mu_all + k->m_pad, k->d_var_all + k->m_pad, k->d_kg, P,
                           ref[0], ref[1], k->m, k->d_acq_sum, k->d_flags, d_trace);
    }, {out_trace, d_trace, trace_len * sizeof(double)}, out_ehvi, out_max, out_argmax, out_flags);
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
    if (st == ROBO_OK)
        st = upload_rows(ctx, "expected hypervolume improvement: upload of the moments",
                         {{k->d_mu, mean2, (size_t)m}, {k->d_q, var2, (size_t)m}});
    if (st == ROBO_OK)
        st = launch_ehvi(ctx, k->d_mean, k->d_var, k->d_mu, k->d_q, k->d_kg, P, ref[0], ref[1], m, k->d_acq_sum, k->d_flags,
                         nullptr);
    return moments_finish(k, st, true, out_ehvi, out_max, out_argmax, out_flags);
}

}  // extern "C"
