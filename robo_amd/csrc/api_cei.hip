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
    for (int i = 0; i < C; ++i) {
        if (!constraints[i]) return ROBO_BAD_ARGUMENT;
        gps.push_back(constraints[i]);
    }
    for (const robo_gp* g : gps)
        if (g->ctx != k->ctx) {
            set_error("%s: the GPs and the candidates must live on one context", CEI_LABEL);
            return ROBO_BAD_ARGUMENT;
        }
    for (size_t i = 0; i < gps.size(); ++i)
        if (gps[i]->dim != k->dim) {
            set_error("%s: GP %d (dim %d) does not match the candidates (dim %d)", CEI_LABEL, (int)i, gps[i]->dim, k->dim);
            return ROBO_BAD_SHAPE;
        }
    for (const robo_gp* g : gps)
        if (!g->fitted) {
            set_error("Model has to be trained first!");
            return ROBO_NOT_FITTED;
        }
    robo_ctx* c = k->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    const size_t trace_len = out_trace ? (size_t)k->m * (2 * (size_t)(C + 1) + 2) : 0;
    ROBO_TRY(dev_grow(c->stream, &k->d_kg, &k->kg_cap, trace_len));
    // the C + 1 sweeps, each chunked by the workspace: row 0 of the handle's sample tables is the objective, row i constraint i
    ROBO_TRY(clear_flags_on_error(k, predict_samples(gps.data(), C + 1, k, C + 1)));
    double* d_trace = out_trace ? k->d_kg : nullptr;
    // event slots 32 -> 33 bracket the fold kernel, under the condition of slots 24..27
    const bool ev = c->phase_events || k->m_pad > 16384;
    if (ev) ROBO_HIP_CHECK(hipEventRecord(c->events[32], c->stream));
    ROBO_TRY(clear_flags_on_error(k, launch_cei(c, k->d_mu_all, k->d_var_all, k->d_mu_all + k->m_pad, k->d_var_all + k->m_pad,
                                                k->m_pad, C, th, acq_kind, par, eta, has_eta != 0, k->m, k->d_acq_sum,
                                                k->d_flags, d_trace)));
    if (ev) ROBO_HIP_CHECK(hipEventRecord(c->events[33], c->stream));
    ROBO_TRY(clear_flags_on_error(k, launch_argmax(k, k->d_acq_sum, 1.0)));
    ROBO_TRY(finish_call(k, CEI_LABEL, ROBO_OK, {{out_trace, d_trace, trace_len * sizeof(double)}}, false));
    // (max, argmax, flags) [+ the values] and the one synchronisation of the call
    return clear_flags_on_error(k, acq_read_back(k, k->d_acq, out_values, out_max, out_argmax, out_flags));
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
    if (st == ROBO_OK && rows > 0) {
        hipError_t e = hipMemcpyAsync(k->d_kg, means, rows * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(k->d_kg + rows, vars, rows * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) {
            set_error("%s: upload of the moments failed: %s", CEI_LABEL, hipGetErrorString(e));
            st = ROBO_RUNTIME_ERROR;
        }
    }
    if (st == ROBO_OK)
        st = launch_cei(ctx, k->d_mean, k->d_var, k->d_kg, k->d_kg + rows, m, C, th, acq_kind, par, eta, has_eta != 0, m,
                        k->d_acq_sum, k->d_flags, nullptr);
    if (st == ROBO_OK) st = launch_argmax(k, k->d_acq_sum, 1.0);
    if (st == ROBO_OK) st = acq_read_back(k, k->d_acq, out_values, out_max, out_argmax, out_flags);
    else hipStreamSynchronize(ctx->stream);
    robo_cand_destroy(k);
    return st;
}

}  // extern "C"
