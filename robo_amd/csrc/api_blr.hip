// C ABI of librobo_hip.so, part 9: Bayesian linear regression on basis features (robo_blr_*; the rule is stated in
// include/robo_hip.h).  Host-side orchestration only: every number is produced by the kernels in blr.hip and acq.hip.
#include <cmath>
#include <vector>

#include "api_internal.h"
#include "blr_dev.h"

namespace robo {
constexpr const char* BLR_LABEL = "Bayesian linear regression";
constexpr int BLR_MAX_PASS = 1024;       // chunk partials in memory at a time, whatever the workspace (128 MB at F = 128)

static void blr_free(robo_blr* h) {
    hipFree(h->d_feat);
    hipFree(h->d_rows);
    hipFree(h->d_part);
    hipFree(h->d_model);
    hipFree(h->d_status);
    hipFree(h->d_hyp);
    hipFree(h->d_ll);
    hipFree(h->d_cand);
    hipFree(h->d_ps);
    if (h->k) robo_cand_destroy(h->k);
    robo_ctx* c = h->ctx;
    delete h;
    ctx_release(c);
}

// the statistics, eigenpairs and hyper-parameter tables of a handle whose feature map is set
static int blr_alloc_model(robo_blr* h) {
    const int FP = h->ft.FP;
    const size_t stats = blr_part_stride(FP), model = stats + (size_t)FP * FP + 2 * FP;
    const size_t hyp = 3 * ROBO_BLR_MAX_SAMPLES + 2 * (size_t)ROBO_BLR_MAX_SAMPLES * FP;
    ROBO_TRY(dev_alloc(&h->d_model, model));
    ROBO_TRY(dev_alloc(&h->d_hyp, hyp));
    ROBO_TRY(dev_alloc(&h->d_status, 2));
    h->d_Qt = h->d_model + stats;
    h->d_lam = h->d_Qt + (size_t)FP * FP;
    h->d_c = h->d_lam + FP;
    h->d_invb = h->d_hyp + 2 * ROBO_BLR_MAX_SAMPLES;
    h->d_wm = h->d_invb + ROBO_BLR_MAX_SAMPLES;
    h->d_wv = h->d_wm + (size_t)ROBO_BLR_MAX_SAMPLES * FP;
    return ROBO_OK;
}

static int blr_ready(const robo_blr* h, bool hypers) {
    if (!h->has_data || (hypers && !h->has_hypers)) {
        set_error("Model has to be trained first!");
        return ROBO_NOT_FITTED;
    }
    return ROBO_OK;
}

// the m candidate rows on the device, the moments' handle sized for them, the sweep launched (asynchronous)
static int blr_sweep(robo_blr* h, const double* rows, int64_t m, bool per_sample) {
    if (!rows || m < 1) {
        set_error("%s: %lld candidates, must be >= 1, with their rows", BLR_LABEL, (long long)m);
        return ROBO_BAD_ARGUMENT;
    }
    ROBO_TRY(blr_ready(h, true));
    robo_ctx* c = h->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    // The moments, the acquisition values and the argmax state are a candidate handle's, so that launch_acq and
    // acq_read_back serve this model as they serve a GP.  The handle's coordinate and solve tables (five m-length arrays)
    // stay unused here, and a change of m costs a synchronisation and a fresh set of allocations: a maximiser keeps one m.
    if (!h->k || h->k->m != m) {
        if (h->k) robo_cand_destroy(h->k);
        h->k = nullptr;
        ROBO_TRY(cand_alloc(c, m, 1, &h->k));
    }
    const size_t len = (size_t)m * blr_row_width(h->ft);
    ROBO_TRY(dev_grow(c->stream, &h->d_cand, &h->cand_cap, len));
    if (per_sample) ROBO_TRY(dev_grow(c->stream, &h->d_ps, &h->ps_cap, (size_t)2 * h->S * (size_t)m));
    ROBO_HIP_CHECK(hipMemcpyAsync(h->d_cand, rows, len * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const bool ev = phase_events_on(c, h->k);        // 30 -> 31: the sweep kernel alone
    if (ev) ROBO_TRY(record_phase(c, EV_FOLD_BEGIN));
    ROBO_TRY(launch_blr_sweep(c, h->ft, h->d_cand, m, h->d_Qt, h->d_wm, h->d_wv, h->d_invb, h->S, h->k->d_mean, h->k->d_var,
                              per_sample ? h->d_ps : nullptr));
    return ev ? record_phase(c, EV_FOLD_END) : ROBO_OK;
}

}  // namespace robo

using namespace robo;

extern "C" {

int32_t robo_blr_create(robo_ctx* ctx, int32_t feat_kind, int32_t dim, int32_t F, const double* omega, const double* phase,
                        double scale, robo_blr** out) {
    if (!ctx || !out) return ROBO_BAD_ARGUMENT;
    if (feat_kind < ROBO_BLR_FEAT_GIVEN || feat_kind > ROBO_BLR_FEAT_RFF || F < 1 || F > ROBO_BLR_MAX_FEATURES || dim < 1 ||
        dim > ROBO_BLR_MAX_DIM) {
        set_error("%s: feature kind %d (0 .. 3), %d features (1 .. %d), dim %d (1 .. %d)", BLR_LABEL, feat_kind, F,
                  ROBO_BLR_MAX_FEATURES, dim, ROBO_BLR_MAX_DIM);
        return ROBO_BAD_ARGUMENT;
    }
    if ((feat_kind == ROBO_BLR_FEAT_LINEAR && F != dim + 1) || (feat_kind == ROBO_BLR_FEAT_QUADRATIC && F != 2 * dim + 1)) {
        set_error("%s: feature kind %d in %d dimensions has %d features, not %d", BLR_LABEL, feat_kind, dim,
                  feat_kind == ROBO_BLR_FEAT_LINEAR ? dim + 1 : 2 * dim + 1, F);
        return ROBO_BAD_ARGUMENT;
    }
    if (feat_kind == ROBO_BLR_FEAT_RFF) {
        bool ok = omega && phase && std::isfinite(scale);
        for (int i = 0; ok && i < dim * F; ++i) ok = std::isfinite(omega[i]);
        for (int i = 0; ok && i < F; ++i) ok = std::isfinite(phase[i]);
        if (!ok) {
            set_error("%s: random Fourier features need finite omega (dim x F), phase (F) and scale", BLR_LABEL);
            return ROBO_BAD_ARGUMENT;
        }
    }
    ROBO_HIP_CHECK(hipSetDevice(ctx->device));
    robo_blr* h = new robo_blr();
    memset(h, 0, sizeof(*h));
    h->ctx = ctx;
    ctx_retain(ctx);
    BlrFeat& ft = h->ft;
    ft.kind = feat_kind;
    ft.dim = dim;
    ft.F = F;
    ft.FP = F <= 16 ? 16 : F <= 32 ? 32 : F <= 64 ? 64 : 128;
    ft.DP = round_up(dim, 4);
    ft.scale = scale;
    const int FP = ft.FP;
    int st = ROBO_OK;
    if (feat_kind == ROBO_BLR_FEAT_RFF) {
        std::vector<double> feat((size_t)ft.DP * FP + FP, 0.0);
        for (int d = 0; d < dim; ++d)
            for (int f = 0; f < F; ++f) feat[(size_t)d * FP + f] = omega[(size_t)d * F + f];
        for (int f = 0; f < F; ++f) feat[(size_t)ft.DP * FP + f] = phase[f];
        st = dev_alloc(&h->d_feat, feat.size());
        if (st == ROBO_OK && hipMemcpy(h->d_feat, feat.data(), feat.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
            st = ROBO_RUNTIME_ERROR;
        ft.omega = h->d_feat;
        ft.phase = h->d_feat + (size_t)ft.DP * FP;
    }
    if (st == ROBO_OK) st = blr_alloc_model(h);
    if (st != ROBO_OK) {
        blr_free(h);
        return st;
    }
    *out = h;
    return ROBO_OK;
}

// kind 4: the features are the last hidden layer of `mlp` and a constant, from a copy of its padded parameters taken here
int32_t robo_blr_create_mlp(robo_ctx* ctx, robo_mlp* mlp, robo_blr** out) {
    if (!ctx || !mlp || !out) return ROBO_BAD_ARGUMENT;
    if (!mlp->has_params) {
        set_error("%s: the network's parameters have to be set first", BLR_LABEL);
        return ROBO_NOT_FITTED;
    }
    if (mlp->ctx->device != ctx->device) {
        set_error("%s: the network lives on device %d, the context on device %d", BLR_LABEL, mlp->ctx->device, ctx->device);
        return ROBO_BAD_ARGUMENT;
    }
    ROBO_HIP_CHECK(hipSetDevice(ctx->device));
    robo_blr* h = new robo_blr();
    memset(h, 0, sizeof(*h));
    h->ctx = ctx;
    ctx_retain(ctx);
    BlrFeat& ft = h->ft;
    ft.kind = ROBO_BLR_FEAT_MLP;
    ft.dim = mlp->net.dim;
    ft.F = mlp->net.H + 1;
    ft.FP = ft.F <= 16 ? 16 : ft.F <= 32 ? 32 : ft.F <= 64 ? 64 : 128;
    ft.DP = mlp->net.DP;
    ft.mlp = mlp->net;
    const size_t len = (size_t)mlp_pad_len(mlp->net);
    int st = dev_alloc(&h->d_feat, len);
    // on the network's own stream, behind its last training call, and complete before anything else can touch either side
    if (st == ROBO_OK && (hipMemcpyAsync(h->d_feat, mlp->d_pad, len * sizeof(double), hipMemcpyDeviceToDevice,
                                         mlp->ctx->stream) != hipSuccess ||
                          hipStreamSynchronize(mlp->ctx->stream) != hipSuccess))
        st = ROBO_RUNTIME_ERROR;
    ft.mlp.pad = h->d_feat;
    if (st == ROBO_OK) st = blr_alloc_model(h);
    if (st != ROBO_OK) {
        blr_free(h);
        return st;
    }
    *out = h;
    return ROBO_OK;
}

int32_t robo_blr_destroy(robo_blr* h) {
    if (!h) return ROBO_OK;
    hipSetDevice(h->ctx->device);
    hipStreamSynchronize(h->ctx->stream);
    blr_free(h);
    return ROBO_OK;
}

int32_t robo_blr_set_data(robo_blr* h, const double* rows, const double* y, int64_t n) {
    if (!h || !rows || !y) return ROBO_BAD_ARGUMENT;
    if (n < 1) {
        set_error("%s: %lld observations, must be >= 1", BLR_LABEL, (long long)n);
        return ROBO_BAD_ARGUMENT;
    }
    robo_ctx* c = h->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    h->has_data = h->has_hypers = false;
    const int FP = h->ft.FP;
    const size_t len = (size_t)n * blr_row_width(h->ft), stride = blr_part_stride(FP);
    const long long chunks = (n + BLR_CHUNK - 1) / BLR_CHUNK;
    // the partials of one pass: what the workspace holds, at least one chunk; the passes continue one sum in chunk order
    long long pass = (long long)(workspace_bytes(c) / (stride * sizeof(double)));
    pass = pass < 1 ? 1 : pass > BLR_MAX_PASS ? BLR_MAX_PASS : pass;
    if (pass > chunks) pass = chunks;
    ROBO_TRY(dev_grow(c->stream, &h->d_rows, &h->rows_cap, len + (size_t)n));
    ROBO_TRY(dev_grow(c->stream, &h->d_part, &h->part_cap, (size_t)pass * stride));
    double* d_y = h->d_rows + len;
    ROBO_HIP_CHECK(hipMemcpyAsync(h->d_rows, rows, len * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ROBO_HIP_CHECK(hipMemcpyAsync(d_y, y, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const bool ev = phase_events_on(c, nullptr);     // 30 -> 31: the statistics and sum kernels; 31 -> 29: the eigensolver
    if (ev) ROBO_TRY(record_phase(c, EV_FOLD_BEGIN));
    for (long long c0 = 0; c0 < chunks; c0 += pass) {
        const int nc = (int)(chunks - c0 < pass ? chunks - c0 : pass);
        ROBO_TRY(launch_blr_stats(c, h->ft, h->d_rows, d_y, n, c0, nc, h->d_part));
        ROBO_TRY(launch_blr_sum(c, h->d_part, nc, FP, c0 == 0, h->d_model));
    }
    if (ev) ROBO_TRY(record_phase(c, EV_FOLD_END));
    ROBO_TRY(launch_blr_eig(c, h->d_model, h->ft.F, FP, h->d_Qt, h->d_lam, h->d_c, h->d_status));
    if (ev) ROBO_TRY(record_phase(c, EV_GRAD_END));
    int status[2] = {1, 0};
    ROBO_HIP_CHECK(hipMemcpyAsync(status, h->d_status, sizeof(status), hipMemcpyDeviceToHost, c->stream));
    ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (status[0] == 2) {
        set_error("%s: the rows or the targets hold a NaN or an infinity", BLR_LABEL);
        return ROBO_BAD_ARGUMENT;
    }
    if (status[0] != 0) {
        set_error("%s: the eigensolver did not converge in %d sweeps", BLR_LABEL, status[1]);
        return ROBO_RUNTIME_ERROR;
    }
    h->n = n;
    h->has_data = true;
    return ROBO_OK;
}

int32_t robo_blr_get_stats(robo_blr* h, double* out_G, double* out_b, double* out_yy, double* out_lambda, double* out_Q) {
    if (!h) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(blr_ready(h, false));
    const int F = h->ft.F, FP = h->ft.FP;
    const size_t stats = blr_part_stride(FP), total = stats + (size_t)FP * FP + 2 * FP;
    std::vector<double> host(total);
    ROBO_HIP_CHECK(hipSetDevice(h->ctx->device));
    ROBO_HIP_CHECK(hipMemcpyAsync(host.data(), h->d_model, total * sizeof(double), hipMemcpyDeviceToHost, h->ctx->stream));
    ROBO_HIP_CHECK(hipStreamSynchronize(h->ctx->stream));
    for (int i = 0; i < F; ++i) {
        for (int j = 0; j < F; ++j) {
            if (out_G) out_G[(size_t)i * F + j] = host[(size_t)i * FP + j];
            if (out_Q) out_Q[(size_t)i * F + j] = host[stats + (size_t)j * FP + i];
        }
        if (out_b) out_b[i] = host[(size_t)FP * FP + i];
        if (out_lambda) out_lambda[i] = host[stats + (size_t)FP * FP + i];
    }
    if (out_yy) *out_yy = host[(size_t)FP * FP + FP];
    return ROBO_OK;
}

int32_t robo_blr_loglik_batch(robo_blr* h, int32_t S, const double* log_alpha_beta, int32_t form, double* out) {
    if (!h || !log_alpha_beta || !out) return ROBO_BAD_ARGUMENT;
    if (S < 1 || form < 0 || form > 1) {
        set_error("%s: %d hyper-parameter pairs (>= 1), likelihood form %d (0 or 1)", BLR_LABEL, S, form);
        return ROBO_BAD_ARGUMENT;
    }
    ROBO_TRY(blr_ready(h, false));
    robo_ctx* c = h->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    ROBO_TRY(dev_grow(c->stream, &h->d_ll, &h->ll_cap, (size_t)3 * S));
    ROBO_HIP_CHECK(hipMemcpyAsync(h->d_ll, log_alpha_beta, (size_t)2 * S * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ROBO_TRY(launch_blr_loglik(c, h->d_model, h->d_lam, h->d_c, h->ft.F, h->ft.FP, h->n, S, h->d_ll, form, h->d_ll + 2 * S));
    ROBO_HIP_CHECK(hipMemcpyAsync(out, h->d_ll + 2 * S, (size_t)S * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));
    return ROBO_OK;
}

int32_t robo_blr_set_hypers(robo_blr* h, int32_t S, const double* alpha_beta) {
    if (!h || !alpha_beta) return ROBO_BAD_ARGUMENT;
    if (S < 1 || S > ROBO_BLR_MAX_SAMPLES) {
        set_error("%s: %d hyper-parameter samples, must be in [1, %d]", BLR_LABEL, S, ROBO_BLR_MAX_SAMPLES);
        return ROBO_BAD_ARGUMENT;
    }
    for (int i = 0; i < 2 * S; ++i)
        if (!std::isfinite(alpha_beta[i]) || !(alpha_beta[i] > 0.0)) {
            set_error("%s: alpha and beta must be positive and finite (sample %d: %g)", BLR_LABEL, i / 2, alpha_beta[i]);
            return ROBO_BAD_ARGUMENT;
        }
    ROBO_TRY(blr_ready(h, false));
    robo_ctx* c = h->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    h->has_hypers = false;
    ROBO_HIP_CHECK(hipMemcpyAsync(h->d_hyp, alpha_beta, (size_t)2 * S * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ROBO_TRY(launch_blr_hypers(c, h->d_lam, h->d_c, h->ft.F, h->ft.FP, S, h->d_hyp, h->d_wm, h->d_wv, h->d_invb));
    ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));        // (the caller's array is free again)
    h->S = S;
    h->has_hypers = true;
    return ROBO_OK;
}

int32_t robo_blr_predict(robo_blr* h, const double* rows, int64_t m, double* out_mean, double* out_var,
                         double* out_per_sample) {
    if (!h || !out_mean || !out_var) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(blr_sweep(h, rows, m, out_per_sample != nullptr));
    const size_t bytes = (size_t)m * sizeof(double);
    return finish_call(h->k, BLR_LABEL, ROBO_OK, {{out_mean, h->k->d_mean, bytes}, {out_var, h->k->d_var, bytes},
                                                  {out_per_sample, h->d_ps, 2 * (size_t)h->S * bytes}});
}

int32_t robo_blr_acq_eval_cand(robo_blr* h, int32_t acq_kind, double par, double eta, const double* rows, int64_t m,
                               double* out_acq, double* out_max, int64_t* out_argmax, uint32_t* out_flags) {
    if (!h) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(check_acq_kind(acq_kind));
    ROBO_TRY(blr_sweep(h, rows, m, false));
    robo_cand* k = h->k;
    ROBO_TRY(clear_flags_on_error(k, launch_acq(h->ctx, k, acq_kind, par, eta, false, false)));
    return clear_flags_on_error(k, acq_read_back(k, k->d_acq, out_acq, out_max, out_argmax, out_flags));
}

}  // extern "C"
