// C ABI of librobo_hip.so, part 7: constrained expected improvement (robo_cei_eval_cand, robo_cei_eval_moments,
// robo_cei_refine_cand; the rules are stated in include/robo_hip.h).  Host-side orchestration only: every number is produced
// by the kernels in predict.hip / cei.hip / acq.hip / refine.hip / cei_refine.hip.
#include <algorithm>
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

// Sweep (robo_cei_eval_cand's, nothing read back) -> the K best folded values become the starts (refine.hip) -> per trial
// and GP the (D + 1)-row solve and cei_refine.hip's epilogue, constraints first, the objective last -> the winner.
// Launches only between the checks and the read-back, which is the one synchronisation of the call.
int32_t robo_cei_refine_cand(robo_gp* objective, robo_gp* const* constraints, int32_t C, const double* thresholds,
                             int32_t acq_kind, double par, double eta, int32_t has_eta, robo_cand* k, int32_t n_starts,
                             int32_t n_steps, double step0, double* out_x, double* out_value, int64_t* out_start_index,
                             uint32_t* out_flags, int64_t* out_starts, double* out_trace) {
    if (!objective || !k || !out_x || (C > 0 && !constraints)) return ROBO_BAD_ARGUMENT;
    CeiThresholds th;
    ROBO_TRY(cei_check(C, thresholds, acq_kind, par, eta, has_eta, &th));
    std::vector<robo_gp*> gps(1, objective);
    gps.insert(gps.end(), constraints, constraints + C);
    ROBO_TRY(models_check(CEI_LABEL, "the GPs", gps.data(), C + 1, k, [&](int i) {
        set_error("%s: GP %d (dim %d) does not match the candidates (dim %d)", CEI_LABEL, i, gps[i]->dim, k->dim);
    }));
    ROBO_TRY(refine_check_steps(n_starts, n_steps, step0));
    for (int i = 0; i <= C; ++i)
        if (gps[i]->kind == ROBO_KERNEL_FABOLAS) {
            set_error("%s: GP %d has a Fabolas kernel, whose fidelity column is not a box coordinate to refine", CEI_LABEL, i);
            return ROBO_BAD_ARGUMENT;
        }
    // the GPs a trial is solved against, in launch order: the constraints, then the objective -- which stays out while there
    // is no incumbent to improve on (with no constraint either its launch still decides, on the constant value)
    std::vector<int> order;
    for (int i = 1; i <= C; ++i) order.push_back(i);
    if (has_eta || C == 0) order.push_back(0);
    robo_ctx* c = k->ctx;
    const int K = n_starts, T = n_steps, D = objective->dim;
    const int64_t rows_pad = round_up64((int64_t)K * (D + 1), NB);
    int n_pad_max = 0;
    for (int i : order) n_pad_max = std::max(n_pad_max, gps[i]->n_pad);
    RefineWork* w = nullptr;
    ROBO_TRY(refine_prepare(objective, n_pad_max, K, T, out_trace != nullptr, &w));      // (state and workspace stay with the objective)
    const RefineState& st = w->st;

    ROBO_TRY(models_fold_launch(gps.data(), C + 1, k, EV_CEI_BEGIN, [&] {
        return launch_cei(c, k->d_mu_all, k->d_var_all, k->d_mu_all + k->m_pad, k->d_var_all + k->m_pad, k->m_pad, C, th,
                          acq_kind, par, eta, has_eta != 0, k->m, k->d_acq_sum, k->d_flags, nullptr);
    }));
    // every GP's solve is decided once, and W built, before the first iteration (refine_core's rule, per GP)
    const bool iterate = T > 0 || out_trace;
    std::vector<char> use_w(gps.size(), 0);
    double* d_rhs = nullptr;
    for (size_t j = 0; iterate && j < order.size(); ++j) {
        robo_gp* g = gps[order[j]];
        bool use = false;
        ROBO_TRY(clear_flags_on_error(k, decide_winv(g, w->ws, &use)));
        use_w[order[j]] = use ? 1 : 0;
        if (use) ROBO_TRY(clear_flags_on_error(k, winv_rows_buffer(g, w->ws, rows_pad, &d_rhs)));   // (grows to the largest)
    }
    int status = launch_refine_select(c, st, k->d_acq, k->m, k->d_Xc, step0);
    for (int t = 0; status == ROBO_OK && iterate && t <= T; ++t) {
        for (size_t j = 0; status == ROBO_OK && j < order.size(); ++j) {
            const int i = order[j];
            robo_gp* g = gps[i];
            const CeiRefineStep step = {i == 0, j == 0, j + 1 == order.size(), i > 0 ? th.t[i - 1] : 0.0, C, acq_kind,
                                        has_eta != 0, par, eta};
            status = launch_refine_solve(g, w, K, use_w[i] ? d_rhs : nullptr);
            if (status == ROBO_OK) status = launch_cei_refine_eval(g, st, w->ws, step, t, T);
        }
    }
    return refine_read_back(k, w, status, T, out_x, out_value, out_start_index, out_flags, out_starts, out_trace);
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
