// C ABI of librobo_hip.so, part 8: the expected hypervolume improvement for two to four objectives over a box
// decomposition (robo_ehvi_box_eval_cand, robo_ehvi_box_eval_moments; the rule is stated in include/robo_hip.h).  Host-side
// orchestration only: every number is produced by the kernels in predict.hip / ehvi_box.hip / acq.hip.
#include <cmath>

#include "api_internal.h"

namespace robo {
constexpr const char* EHVI_BOX_LABEL = "expected hypervolume improvement (boxes)";

// the bounds and boxes as the rule needs them -> the kernel's row layout
static int ehvi_box_check(int64_t K, const double* bounds, const int32_t* n_bounds, const uint16_t* boxes, int64_t B,
                          EhviBoxShape* sh) {
    if (K < 2 || K > ROBO_EHVI_BOX_MAX_OBJ || !bounds || !n_bounds || !boxes) {
        set_error("%s: %lld objectives, must be in [2, %d], with their bounds and boxes", EHVI_BOX_LABEL, (long long)K,
                  ROBO_EHVI_BOX_MAX_OBJ);
        return ROBO_BAD_ARGUMENT;
    }
    if (B < 1 || B > ROBO_EHVI_BOX_MAX_BOXES) {
        set_error("%s: %lld boxes, must be in [1, %d]", EHVI_BOX_LABEL, (long long)B, ROBO_EHVI_BOX_MAX_BOXES);
        return ROBO_BAD_ARGUMENT;
    }
    sh->K = (int)K;
    sh->rows = 0;
    for (int k = 0; k < ROBO_EHVI_BOX_MAX_OBJ; ++k) {
        sh->base[k] = sh->rows;
        if (k >= K) continue;
        const int n = n_bounds[k];
        if (n < 2 || n > ROBO_EHVI_BOX_MAX_BOUNDS) {
            set_error("%s: objective %d has %d bounds, must be in [2, %d]", EHVI_BOX_LABEL, k, n, ROBO_EHVI_BOX_MAX_BOUNDS);
            return ROBO_BAD_ARGUMENT;
        }
        const double* t = bounds + sh->rows;
        if (!(std::isinf(t[0]) && t[0] < 0.0)) {
            set_error("%s: the first bound of objective %d is %g, not -inf", EHVI_BOX_LABEL, k, t[0]);
            return ROBO_BAD_ARGUMENT;
        }
        for (int j = 1; j < n; ++j)
            if (!std::isfinite(t[j]) || !(t[j - 1] < t[j])) {
                set_error("%s: bound %d of objective %d = %g is not finite and above bound %d = %g", EHVI_BOX_LABEL, j, k,
                          t[j], j - 1, t[j - 1]);
                return ROBO_BAD_ARGUMENT;
            }
        sh->rows += n;
    }
    for (int64_t b = 0; b < B; ++b)
        for (int k = 0; k < K; ++k) {
            const int lo = boxes[(b * K + k) * 2], hi = boxes[(b * K + k) * 2 + 1];
            if (lo >= hi || hi >= n_bounds[k]) {
                set_error("%s: box %lld spans bounds [%d, %d) of objective %d, which has %d", EHVI_BOX_LABEL, (long long)b,
                          lo, hi, k, n_bounds[k]);
                return ROBO_BAD_ARGUMENT;
            }
        }
    return ROBO_OK;
}

// [bounds (rows) | box words (B x K, two to a double) | extra] in the handle's diagnostics buffer, bounds and boxes uploaded
// (asynchronous: the caller's arrays outlive the call's synchronisation) -> the three parts
struct EhviBoxStage {
    double* bounds;
    unsigned* boxes;
    double* extra;
};
static int ehvi_box_stage(robo_cand* k, const EhviBoxShape& sh, const double* bounds, const uint16_t* boxes, int B,
                          size_t extra_len, EhviBoxStage* out) {
    const size_t words = (size_t)B * sh.K, box_len = (words + 1) / 2;
    ROBO_TRY(dev_grow(k->ctx->stream, &k->d_kg, &k->kg_cap, (size_t)sh.rows + box_len + extra_len));
    out->bounds = k->d_kg;
    out->boxes = reinterpret_cast<unsigned*>(k->d_kg + sh.rows);
    out->extra = k->d_kg + sh.rows + box_len;
    ROBO_HIP_CHECK(hipMemcpyAsync(out->bounds, bounds, (size_t)sh.rows * sizeof(double), hipMemcpyHostToDevice, k->ctx->stream));
    ROBO_HIP_CHECK(hipMemcpyAsync(out->boxes, boxes, words * sizeof(unsigned), hipMemcpyHostToDevice, k->ctx->stream));
    return ROBO_OK;
}

}  // namespace robo

using namespace robo;

extern "C" {

int32_t robo_ehvi_box_eval_cand(robo_gp* const* gps, int32_t K, robo_cand* k, const double* bounds, const int32_t* n_bounds,
                                const uint16_t* boxes, int32_t B, double* out_ehvi, double* out_max, int64_t* out_argmax,
                                uint32_t* out_flags, double* out_trace) {
    if (!gps || !k) return ROBO_BAD_ARGUMENT;
    EhviBoxShape sh;
    ROBO_TRY(ehvi_box_check(K, bounds, n_bounds, boxes, B, &sh));
    ROBO_TRY(models_check(EHVI_BOX_LABEL, "the GPs", gps, K, k, [&](int i) {
        set_error("%s: GP %d (dim %d) does not match the candidates (dim %d)", EHVI_BOX_LABEL, i, gps[i]->dim, k->dim);
    }));
    const size_t trace_len = out_trace ? (size_t)k->m * 2 * (size_t)K : 0;
    EhviBoxStage st;
    ROBO_TRY(ehvi_box_stage(k, sh, bounds, boxes, B, trace_len, &st));
    double* d_trace = out_trace ? st.extra : nullptr;
    // objective i is row i of the handle's sample tables; slots 34 -> 35 bracket the box kernel
    return models_fold(EHVI_BOX_LABEL, gps, K, k, EV_EHVI_BOX_BEGIN, [&] {
        return launch_ehvi_box(k->ctx, k->d_mu_all, k->d_var_all, k->m_pad, sh, st.bounds, st.boxes, B, k->m, k->d_acq_sum,
                               k->d_flags, d_trace);
    }, {out_trace, d_trace, trace_len * sizeof(double)}, out_ehvi, out_max, out_argmax, out_flags);
}

int32_t robo_ehvi_box_eval_moments(robo_ctx* ctx, int64_t m, int32_t K, const double* mean, const double* var,
                                   const double* bounds, const int32_t* n_bounds, const uint16_t* boxes, int32_t B,
                                   double* out_ehvi, double* out_max, int64_t* out_argmax, uint32_t* out_flags) {
    if (!ctx || !mean || !var) return ROBO_BAD_ARGUMENT;
    EhviBoxShape sh;
    ROBO_TRY(ehvi_box_check(K, bounds, n_bounds, boxes, B, &sh));
    const char* what = "expected hypervolume improvement (boxes): upload of the moments";
    robo_cand* k = nullptr;
    ROBO_TRY(cand_alloc(ctx, m, 1, &k));          // (the handle's own mean / var rows stay unused: all K rows go to d_kg)
    // [means (K x m) | vars (K x m)] behind the bounds and the boxes in the handle's diagnostics buffer
    const size_t rows = (size_t)K * (size_t)m;
    EhviBoxStage st;
    int status = ehvi_box_stage(k, sh, bounds, boxes, B, 2 * rows, &st);
    if (status == ROBO_OK) status = upload_rows(ctx, what, {{st.extra, mean, rows}, {st.extra + rows, var, rows}});
    if (status == ROBO_OK)
        status = launch_ehvi_box(ctx, st.extra, st.extra + rows, m, sh, st.bounds, st.boxes, B, m, k->d_acq_sum, k->d_flags,
                                 nullptr);
    return moments_finish(k, status, true, out_ehvi, out_max, out_argmax, out_flags);
}

}  // extern "C"
