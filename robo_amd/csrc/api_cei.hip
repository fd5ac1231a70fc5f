// C ABI of librobo_hip.so, part 7: constrained expected improvement (robo_cei_eval_cand, robo_cei_eval_moments; the rule is
// stated in include/robo_hip.h).  Host-side orchestration only: every number is produced by the kernels in predict.hip /
// cei.hip / acq.hip.
#include <cmath>
#include <vector>

#include "api_internal.h"

namespace robo {
constexpr const char* CEI_LABEL = "constrained expected improvement";

// what both entry points take besides their models or moments: 0 <= C <= ROBO_CEI_MAX_CONSTRAINTS finite thresholds, EI or
// LogEI, and with has_eta a finite incumbent value and exploration parameter -> the thresholds as the kernel takes them
static int cei_check(int64_t C, const double* thresholds, int acq_kind, double par, double eta, int has_eta,
                     CeiThresholds* th) {
    if (C < 0 || C > ROBO_CEI_MAX_CONSTRAINTS || (C > 0 && !thresholds)) {
        set_error("%s: %lld constraints, must be in [0, %d], with their thresholds", CEI_LABEL, (long long)C,
                  ROBO_CEI_MAX_CONSTRAINTS);
        return ROBO_BAD_ARGUMENT;
    }
    if (acq_kind != ROBO_ACQ_EI && acq_kind != ROBO_ACQ_LOG_EI) {
        set_error("%s: acquisition kind %d is neither EI nor LogEI", CEI_LABEL, acq_kind);
        return ROBO_BAD_ARGUMENT;
    }
    for (int k = 0; k < ROBO_CEI_MAX_CONSTRAINTS; ++k) th->t[k] = 0.0;
    for (int64_t k = 0; k < C; ++k) {
        if (!std::isfinite(thresholds[k])) {
            set_error("%s: threshold %lld = %g is not finite", CEI_LABEL, (long long)k, thresholds[k]);
            return ROBO_BAD_ARGUMENT;
        }
        th->t[k] = thresholds[k];
    }
    if (has_eta && (!std::isfinite(eta) || !std::isfinite(par))) {
        set_error("%s: eta = %g, par = %g must be finite (has_eta = 0 says that there is no feasible incumbent)", CEI_LABEL,
                  eta, par);
        return ROBO_BAD_ARGUMENT;
    }
    return ROBO_OK;
}

}  // namespace robo

using namespace robo;

extern "C" {

int32_t robo_cei_eval_cand(robo_gp* objective, robo_gp* const* constraints, int32_t C, const double* thresholds,
                           int32_t acq_kind, double par, double eta, int32_t has_eta, robo_cand* k, double* out_values,
                           double* out_max, int64_t* out_argmax, uint32_t* out_flags, double* out_trace) {
    if (!objective || !k || (C > 0 && !constraints)) return ROBO_BAD_ARGUMENT;
    CeiThresholds th;
    ROBO_TRY(cei_check(C, thresholds, acq_kind, par, eta, has_eta, &th));
    std::vector<robo_gp*> gps(1, objective);
    gps.insert(gps.end(), constraints, constraints + C);
    ROBO_TRY(models_check(CEI_LABEL, "the GPs", gps.data(), C + 1, k, [&](int i) {
        set_error("%s: GP %d (dim %d) does not match the candidates (dim %d)", CEI_LABEL, i, gps[i]->dim, k->dim);
    }));
    const size_t trace_len = out_trace ? (size_t)k->m * (2 * (size_t)(C + 1) + 2) : 0;
    ROBO_TRY(dev_grow(k->ctx->stream, &k->d_kg, &k->kg_cap, trace_len));
    double* d_trace = out_trace ? k->d_kg : nullptr;
    // row 0 of the handle's sample tables is the objective, row i constraint i; slots 32 -> 33 bracket the fold kernel
    return models_fold(CEI_LABEL, gps.data(), C + 1, k, EV_CEI_BEGIN, [&] {
        return launch_cei(k->ctx, k->d_mu_all, k->d_var_all, k->d_mu_all + k->m_pad, k->d_var_all + k->m_pad, k->m_pad, C, th,
                          acq_kind, par, eta, has_eta != 0, k->m, k->d_acq_sum, k->d_flags, d_trace);
    }, {out_trace, d_trace, trace_len * sizeof(double)}, out_values, out_max, out_argmax, out_flags);
}

int32_t robo_cei_eval_moments(robo_ctx* ctx, int64_t m, int32_t C, const double* mean0, const double* var0,
                              const double* means, const double* vars, const double* thresholds, int32_t acq_kind,
                              double par, double eta, int32_t has_eta, double* out_values, double* out_max,
                              int64_t* out_argmax, uint32_t* out_flags) {
    if (!ctx || !mean0 || !var0 || (C > 0 && (!means || !vars))) return ROBO_BAD_ARGUMENT;
    CeiThresholds th;
    ROBO_TRY(cei_check(C, thresholds, acq_kind, par, eta, has_eta, &th));
    robo_cand* k = nullptr;
    ROBO_TRY(moments_handle(ctx, mean0, var0, m, "constrained expected improvement: upload of the moments", &k));
    // the constraints' moments: [means (C x m) | vars (C x m)] in the handle's diagnostics buffer
    const size_t rows = (size_t)C * (size_t)m;
    int st = dev_grow(ctx->stream, &k->d_kg, &k->kg_cap, 2 * rows);
    if (st == ROBO_OK)
        st = upload_rows(ctx, "constrained expected improvement: upload of the moments",
                         {{k->d_kg, means, rows}, {k->d_kg + rows, vars, rows}});
    if (st == ROBO_OK)
        st = launch_cei(ctx, k->d_mean, k->d_var, k->d_kg, k->d_kg + rows, m, C, th, acq_kind, par, eta, has_eta != 0, m,
                        k->d_acq_sum, k->d_flags, nullptr);
    return moments_finish(k, st, true, out_values, out_max, out_argmax, out_flags);
}

}  // extern "C"
