// C ABI of librobo_hip.so, part 2: GP handles, their data, the fit (single theta, batched, the device-resident
// hyper-parameter chain) and the factor read-backs.  Host-side orchestration only: every number is produced by the
// kernels in gram.hip / potrf.hip / mcmc.hip.
#include <atomic>
#include <cmath>
#include <functional>
#include <vector>

#include "api_internal.h"

using namespace robo;

extern "C" {

int32_t robo_gp_create(robo_ctx* ctx, int32_t kind, int32_t n_max, int32_t dim, robo_gp** out) {
    if (!ctx || !out) return ROBO_BAD_ARGUMENT;
    if (kind != ROBO_KERNEL_MATERN52_ARD && kind != ROBO_KERNEL_RBF_ARD && kind != ROBO_KERNEL_FABOLAS) {
        set_error("unknown kernel kind %d", kind);
        return ROBO_BAD_ARGUMENT;
    }
    if (n_max < 1 || dim < 1 || dim > MAX_DIM || (kind == ROBO_KERNEL_FABOLAS && dim < 2)) {
        set_error("bad shape n_max=%d dim=%d (dim <= %d)", n_max, dim, MAX_DIM);
        return ROBO_BAD_SHAPE;
    }
    ROBO_HIP_CHECK(hipSetDevice(ctx->device));
    robo_gp* g = new robo_gp();
    memset(g, 0, sizeof(*g));
    g->ctx = ctx;
    g->kind = kind;
    g->dim = dim;
    g->n_max = n_max;
    g->n_pad_max = round_up(n_max + 1, NB);
    g->y_mean = 0.0;
    g->y_std = 1.0;
    const size_t np = (size_t)g->n_pad_max;
    ROBO_TRY(dev_alloc(&g->d_X, (size_t)n_max * dim));
    ROBO_TRY(dev_alloc(&g->d_Xs, np * dim));
    ROBO_TRY(dev_alloc(&g->d_y, (size_t)n_max));
    ROBO_TRY(dev_alloc(&g->d_K, np * np));
    ROBO_TRY(dev_alloc(&g->d_Linv, np * NB));
    // the strictly upper 16x16 sub-blocks of every inverted diagonal block are zero and never written
    ROBO_HIP_CHECK(hipMemset(g->d_Linv, 0, np * NB * sizeof(double)));
    ROBO_TRY(dev_alloc(&g->d_LinvP, (np / NB) * WP_BLOCK));
    ROBO_HIP_CHECK(hipMemset(g->d_LinvP, 0, (np / NB) * WP_BLOCK * sizeof(double)));
    ROBO_TRY(dev_alloc(&g->d_llpart, (np / NB) * 4));
    ROBO_TRY(dev_alloc(&g->d_theta, (size_t)dim + 8 + sizeof(FitSample) / sizeof(double) + (size_t)dim));
    g->d_sp = reinterpret_cast<FitSample*>(g->d_theta + dim + 8);
    g->d_x2max = g->d_theta + dim + 8 + sizeof(FitSample) / sizeof(double);
    ctx_retain(ctx);
    *out = g;
    return ROBO_OK;
}

int32_t robo_gp_destroy(robo_gp* g) {
    if (!g) return ROBO_OK;
    hipSetDevice(g->ctx->device);
    hipStreamSynchronize(g->ctx->stream);
    robo_cand_destroy(g->host_cand);
    if (g->refine) {
        robo_cand_destroy(g->refine->ws);
        refine_free(g->refine);
    }
    batch_free(g->batch);
    qei_free(g->qei);
    mes_free(g->mes);
    rep_free(g->rep);
    hyper_free(g->hyper);
    hipFree(g->d_X);
    hipFree(g->d_Xs);
    hipFree(g->d_y);
    hipFree(g->d_K);
    hipFree(g->d_Linv);
    hipFree(g->d_LinvP);
    hipFree(g->d_llpart);
    hipFree(g->d_bllpart);
    hipFree(g->d_bkeep);
    hipFree(g->d_theta);
    hipFree(g->d_Winv);
    hipFree(g->d_alpha);
    hipFree(g->d_wnorm);
    if (g->h_wnorm) hipHostFree(g->h_wnorm);
    hipFree(g->d_mcmc);
    for (int v = 0; v < 3; ++v) {
        hipFree(g->d_wunits[v]);
        hipFree(g->d_wprefix[v]);
    }
    hipFree(g->d_gV);
    hipFree(g->d_gA);
    hipFree(g->d_galpha);
    hipFree(g->d_gpart);
    hipFree(g->d_gout);
    hipFree(g->d_bK);
    hipFree(g->d_bLinv);
    hipFree(g->d_bXs);
    hipFree(g->d_bout);
    hipFree(g->d_bsp);
    hipFree(g->d_bfail);
    hipFree(g->d_bprog);
    if (g->h_bstage) hipHostFree(g->h_bstage);
    robo_ctx* ctx = g->ctx;
    delete g;
    ctx_release(ctx);
    return ROBO_OK;
}

int32_t robo_gp_set_data(robo_gp* g, const double* X, const double* y, int32_t n) {
    if (!g || !X || !y) return ROBO_BAD_ARGUMENT;
    if (n < 1 || n > g->n_max) {
        set_error("n=%d outside [1, n_max=%d]", n, g->n_max);
        return ROBO_BAD_SHAPE;
    }
    robo_ctx* c = g->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    ROBO_HIP_CHECK(hipMemcpyAsync(g->d_X, X, (size_t)n * g->dim * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ROBO_HIP_CHECK(hipMemcpyAsync(g->d_y, y, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    // the data extents that decide between the two fp64 gram tiles (common.h gram_needs_direct)
    for (int d = 0; d < g->dim; ++d) g->x2max[d] = 0.0;
    for (int i = 0; i < n; ++i)
        for (int d = 0; d < g->dim; ++d) {
            const double x = X[(size_t)i * g->dim + d], x2 = x * x;
            if (x2 > g->x2max[d]) g->x2max[d] = x2;
        }
    ROBO_HIP_CHECK(hipMemcpyAsync(g->d_x2max, g->x2max, (size_t)g->dim * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (n % NB == 0) {
        // the augmented row's own block (block n / NB) is never factored nor inverted (launch_potrf): its inverse slots
        // must not carry a former data set's entries -- the pack / keep kernels copy every block of the padded range
        const size_t blk = (size_t)(n / NB);
        ROBO_HIP_CHECK(hipMemsetAsync(g->d_Linv + blk * NB * NB, 0, (size_t)NB * NB * sizeof(double), c->stream));
        ROBO_HIP_CHECK(hipMemsetAsync(g->d_LinvP + blk * WP_BLOCK, 0, (size_t)WP_BLOCK * sizeof(double), c->stream));
    }
    ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));
    g->n = n;
    g->n_pad = round_up(n + 1, NB);
    g->has_data = true;
    g->fitted = false;
    return ROBO_OK;
}

int32_t robo_theta_size(int32_t kind, int32_t dim) { return kind == ROBO_KERNEL_FABOLAS ? dim + 3 : dim + 2; }

int32_t robo_gp_set_precision(robo_gp* g, int32_t fp32_gram) {
    if (!g) return ROBO_BAD_ARGUMENT;
    g->fp32_gram = fp32_gram != 0;
    g->fitted = false;
    return ROBO_OK;
}

int32_t robo_gp_set_output_transform(robo_gp* g, double y_mean, double y_std) {
    if (!g) return ROBO_BAD_ARGUMENT;
    g->y_mean = y_mean;
    g->y_std = y_std;
    return ROBO_OK;
}

}  // extern "C"

namespace robo {
// theta -> (FitSample, 1/sqrt(metric_d)); returns BAD_ARGUMENT for non-finite entries
int theta_to_sample(const robo_gp* g, const double* theta, double mean_c, FitSample* sp, double* ism) {
    const int D = g->dim, P = robo_theta_size(g->kind, D);
    for (int p = 0; p < P; ++p)
        if (!std::isfinite(theta[p])) {
            set_error("theta[%d] is not finite", p);
            return ROBO_BAD_ARGUMENT;
        }
    const bool fab = g->kind == ROBO_KERNEL_FABOLAS;
    const int n_metric = fab ? D - 1 : D;
    for (int d = 0; d < n_metric; ++d) ism[d] = std::exp(-0.5 * theta[1 + d]);   // 1/sqrt(metric_d)
    if (fab) ism[D - 1] = 1.0;   // the fidelity column enters the linear kernel unscaled
    sp->cov.kind = g->kind;
    sp->cov.dim = D;
    sp->cov.amp = std::exp(theta[0]);
    sp->cov.blr_a = fab ? std::exp(theta[D]) : 0.0;
    sp->cov.blr_b = fab ? std::exp(theta[D + 1]) : 0.0;
    sp->noise = std::exp(theta[P - 1]) + JITTER;
    sp->mean_c = mean_c;
    sp->direct = gram_needs_direct(g->kind, ism, g->x2max, D);
    return ROBO_OK;
}
}  // namespace robo

extern "C" {

static unsigned long long next_fit_gen() {
    static std::atomic<unsigned long long> gen{0};   // contexts of several devices fit on their own threads (multi.hip)
    return ++gen;
}

static FitBuffers own_buffers(robo_gp* g) {
    FitBuffers fb;
    fb.K = g->d_K; fb.k_stride = 0;
    fb.Linv = g->d_Linv; fb.linv_stride = 0;
    fb.Xs = g->d_Xs; fb.xs_stride = 0;
    fb.sp = g->d_sp;
    fb.fail = g->ctx->d_fail;
    fb.prog = g->ctx->d_prog;
    fb.out = g->ctx->d_scalars;
    fb.ll_part = g->d_llpart;
    fb.LinvP = g->d_LinvP;
    fb.host_out = g->ctx->h_pinned;
    fb.want_inverse = true;
    fb.skip_tail = false;
    fb.S = 1;
    return fb;
}

// stage theta, scale inputs, build the gram matrix into the GP's own buffers (asynchronous)
static int gp_build_gram(robo_gp* g, const double* theta, double mean_c) {
    robo_ctx* c = g->ctx;
    const int D = g->dim;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    ThetaArgs ta = {};
    ROBO_TRY(theta_to_sample(g, theta, mean_c, &ta.sp, ta.ism));
    g->cov = ta.sp.cov;
    g->amp = ta.sp.cov.amp;
    g->noise = ta.sp.noise;
    g->mean_c = mean_c;
    // theta travels as kernel arguments; block 0 of the scaling kernel leaves d_theta (metrics) and d_sp behind
    ROBO_TRY(launch_scale_inputs_theta(c, g->d_X, g->d_Xs, ta, g->n, g->n_pad, D, g->d_theta, g->d_sp));
    if (phase_events_on(c, nullptr)) ROBO_TRY(record_phase(c, EV_GRAM_KERNEL));   // 19 -> 21: the gram kernel alone (K1)
    FitBuffers fb = own_buffers(g);
    fb.gram_mixed = ta.sp.direct != 0;
    ROBO_TRY(launch_gram(g, fb));
    return ROBO_OK;
}

int32_t robo_gp_fit(robo_gp* g, const double* theta, double mean_c, double* out_loglik, int32_t* out_fail_col) {
    if (!g || !theta) return ROBO_BAD_ARGUMENT;
    if (!g->has_data) {
        set_error("robo_gp_fit before robo_gp_set_data");
        return ROBO_NOT_FITTED;
    }
    robo_ctx* c = g->ctx;
    g->fitted = false;
    // event slots 20..23: 20 -> 21 gram build, 21 -> 22 Cholesky, 22 -> 23 log-likelihood reduce
    const bool ev = phase_events_on(c, nullptr);
    if (ev) ROBO_TRY(record_phase(c, EV_FIT_BEGIN));
    ROBO_TRY(gp_build_gram(g, theta, mean_c));
    if (ev) ROBO_TRY(record_phase(c, EV_FIT_GRAM_END));
    ROBO_TRY(launch_potrf(g, own_buffers(g)));
    if (ev) ROBO_TRY(record_phase(c, EV_FIT_POTRF_END));
    if (ev) ROBO_TRY(record_phase(c, EV_FIT_END));
    // the tail kernel of the factorisation wrote (z.z, log det, failure flag) straight into the pinned buffer
    double* hp = c->h_pinned;
    ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));
    const int fail = (int)hp[2];
    if (fail < 0) {
        // a panel follower's bounded poll ran out (potrf.hip panel_follow): a workgroup of the step kernel never saw the
        // diagonal workgroup's progress -- not a property of the matrix
        if (out_loglik) *out_loglik = -HUGE_VAL;
        set_error("factorisation hand-off timed out (tuning potrf_follow=0 selects the launch-per-phase form)");
        return ROBO_RUNTIME_ERROR;
    }
    if (fail != 0) {
        if (out_fail_col) *out_fail_col = fail - 1;
        if (out_loglik) *out_loglik = -HUGE_VAL;
        set_error("matrix is not positive definite (column %d)", fail - 1);
        return ROBO_NOT_POSITIVE_DEFINITE;
    }
    const double quad = hp[0], logdet = hp[1];
    g->diag_min = hp[3];
    g->diag_max = hp[4];
    g->loglik = -0.5 * (quad + logdet + (double)g->n * std::log(2.0 * M_PI));
    g->fitted = true;
    g->fit_gen = next_fit_gen();
    if (out_loglik) *out_loglik = g->loglik;
    if (out_fail_col) *out_fail_col = -1;
    return ROBO_OK;
}

int32_t robo_gp_grad_loglik(robo_gp* g, const double* theta, double mean_c, double* out_loglik, double* out_grad,
                            int32_t* out_fail_col) {
    if (!g || !theta || !out_grad) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(robo_gp_fit(g, theta, mean_c, out_loglik, out_fail_col));
    robo_ctx* c = g->ctx;
    const int P = robo_theta_size(g->kind, g->dim);
    if (!g->d_gV) ROBO_TRY(dev_alloc(&g->d_gV, (size_t)g->n_pad_max * g->n_pad_max));   // (shared with winv_ensure)
    if (!g->d_gA) {
        const size_t np = (size_t)g->n_pad_max, t64 = (np + 63) / 64;
        ROBO_TRY(dev_alloc(&g->d_gA, np * np));
        ROBO_TRY(dev_alloc(&g->d_galpha, np));
        ROBO_TRY(dev_alloc(&g->d_gpart, (size_t)P * (t64 * (t64 + 1) / 2)));
        ROBO_TRY(dev_alloc(&g->d_gout, (size_t)P));
    }
    // event slots 28 -> 29: everything after the factorisation (W^T, A, the reductions)
    ROBO_TRY(record_phase(c, EV_GRAD_BEGIN));
    double* hg = c->h_pinned + 8;          // P <= MAX_DIM + 3 doubles behind the fit's three result slots
    ROBO_TRY(launch_grad_loglik(g, g->d_gV, g->d_gA, g->d_galpha, g->d_gpart, g->d_gout, hg));
    ROBO_TRY(record_phase(c, EV_GRAD_END));
    ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));
    memcpy(out_grad, hg, (size_t)P * sizeof(double));
    return ROBO_OK;
}

}  // extern "C"

namespace robo {
// grow the batch workspace to hold S samples at the current n_pad
int batch_ensure(robo_gp* g, int S) {
    if (g->b_cap >= S && g->b_npad == g->n_pad) return ROBO_OK;
    hipFree(g->d_bK); hipFree(g->d_bLinv); hipFree(g->d_bXs); hipFree(g->d_bout);
    hipFree(g->d_bsp); hipFree(g->d_bfail); hipFree(g->d_bllpart); hipFree(g->d_bkeep);   // d_bism lives in d_bsp's block
    hipFree(g->d_bprog);
    g->d_bprog = nullptr;
    if (g->h_bstage) hipHostFree(g->h_bstage);
    g->d_bK = g->d_bLinv = g->d_bXs = g->d_bism = g->d_bout = g->h_bstage = nullptr;
    g->d_bsp = nullptr; g->d_bfail = nullptr; g->d_bllpart = nullptr; g->d_bkeep = nullptr;
    g->b_cap = 0;
    const size_t np = (size_t)g->n_pad, D = (size_t)g->dim;
    ROBO_TRY(dev_alloc(&g->d_bK, (size_t)S * np * np));
    ROBO_TRY(dev_alloc(&g->d_bLinv, (size_t)S * np * NB));
    ROBO_HIP_CHECK(hipMemset(g->d_bLinv, 0, (size_t)S * np * NB * sizeof(double)));
    ROBO_TRY(dev_alloc(&g->d_bXs, (size_t)S * np * D));
    ROBO_TRY(dev_alloc(&g->d_bout, (size_t)S * 2));
    {   // [S x FitSample | S x D inverse sqrt metrics] in one block: one upload per pass
        char* blk = nullptr;
        ROBO_TRY(dev_alloc(&blk, (size_t)S * sizeof(FitSample) + (size_t)S * D * sizeof(double)));
        g->d_bsp = reinterpret_cast<FitSample*>(blk);
        g->d_bism = reinterpret_cast<double*>(g->d_bsp + S);
    }
    ROBO_TRY(dev_alloc(&g->d_bfail, (size_t)S));
    ROBO_TRY(dev_alloc(&g->d_bprog, (size_t)S * PROG_STRIDE));
    ROBO_TRY(dev_alloc(&g->d_bllpart, (size_t)S * (np / NB) * 4));
    ROBO_TRY(dev_alloc(&g->d_bkeep, (size_t)S * sizeof(KeepDst)));
    // pinned staging: [S x FitSample | S x D ism] up, [S x 5 doubles] down (written by the device)
    const size_t bytes = (size_t)S * (sizeof(FitSample) + D * sizeof(double) + 5 * sizeof(double)) + 64;
    ROBO_HIP_CHECK(hipHostMalloc((void**)&g->h_bstage, bytes, 0));
    g->b_cap = S;
    g->b_npad = g->n_pad;
    return ROBO_OK;
}
}  // namespace robo

extern "C" {

// S thetas on the training data of g, factorised by ONE sequence of launches per workspace chunk.  After each
// chunk `keep(s0, ns, status)` may copy the chunk's factors out of the strided batch workspace (it runs before
// the next chunk overwrites them).
static int fit_batch_core(robo_gp* g, const double* thetas, int32_t S, double mean_c, double* out_loglik,
                          int32_t* out_status, const std::function<int(int, int, const int*)>& keep) {
    robo_ctx* c = g->ctx;
    const int P = robo_theta_size(g->kind, g->dim), D = g->dim;
    const size_t np = (size_t)g->n_pad;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    // bound the workspace: sub-batches of at most `chunk` samples (S * n_pad^2 doubles each)
    size_t per = np * np * sizeof(double) + np * (NB + (size_t)D) * sizeof(double);
    int chunk = (int)(workspace_bytes(c) / per);
    if (chunk < 1) chunk = 1;
    if (chunk > S) chunk = S;
    ROBO_TRY(batch_ensure(g, chunk));
    for (int s0 = 0; s0 < S; s0 += chunk) {
        const int ns = S - s0 < chunk ? S - s0 : chunk;
        ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));   // staging buffer reuse
        const int cap = g->b_cap;                          // layout of the staging block and of its device twin
        FitSample* hsp = reinterpret_cast<FitSample*>(g->h_bstage);
        double* hism = reinterpret_cast<double*>(hsp + cap);
        double* hout = hism + (size_t)cap * D;             // [ns][5]: z.z, log det, failure flag, min / max L_ii
        std::vector<int> status(ns, ROBO_OK);
        bool any_direct = false;
        for (int s = 0; s < ns; ++s) {
            const int st = theta_to_sample(g, thetas + (size_t)(s0 + s) * P, mean_c, hsp + s, hism + (size_t)s * D);
            status[s] = st;
            if (st != ROBO_OK) {   // keep the slot numerically harmless: unit kernel
                static const double zeros[MAX_DIM + 8] = {0};
                theta_to_sample(g, zeros, mean_c, hsp + s, hism + (size_t)s * D);
            }
            if (hsp[s].direct) any_direct = true;
        }
        ROBO_HIP_CHECK(hipMemcpyAsync(g->d_bsp, hsp, (size_t)cap * sizeof(FitSample) + (size_t)ns * D * sizeof(double),
                                      hipMemcpyHostToDevice, c->stream));
        FitBuffers fb;
        fb.K = g->d_bK; fb.k_stride = np * np;
        fb.prog = g->d_bprog;
        fb.Linv = g->d_bLinv; fb.linv_stride = np * NB;
        fb.Xs = g->d_bXs; fb.xs_stride = np * D;
        fb.sp = g->d_bsp;
        fb.fail = g->d_bfail;
        fb.out = g->d_bout;
        fb.ll_part = g->d_bllpart;
        fb.LinvP = nullptr;
        fb.host_out = hout;
        fb.want_inverse = (bool)keep;      // likelihoods only: the posterior's inverse blocks are not formed
        fb.skip_tail = false;
        fb.gram_mixed = any_direct;
        fb.S = ns;
        ROBO_TRY(launch_scale_inputs(c, g->d_X, g->d_bXs, g->d_bism, g->n, g->n_pad, D, ns, np * D, (size_t)D));
        ROBO_TRY(launch_potrf(g, fb, true));   // gram + factorisation; its tail kernel also reduces the log-likelihood terms into fb.out
        ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));   // the finishing kernel wrote hout (pinned) itself
        for (int s = 0; s < ns; ++s) {
            double ll = -HUGE_VAL;
            if (status[s] == ROBO_OK) {
                if (hout[5 * s + 2] < 0.0) status[s] = ROBO_RUNTIME_ERROR;      // a follower's hand-off timed out (potrf.hip)
                else if (hout[5 * s + 2] != 0.0) status[s] = ROBO_NOT_POSITIVE_DEFINITE;
                else ll = -0.5 * (hout[5 * s] + hout[5 * s + 1] + (double)g->n * std::log(2.0 * M_PI));
            }
            out_loglik[s0 + s] = ll;
            if (out_status) out_status[s0 + s] = status[s];
        }
        if (keep) ROBO_TRY(keep(s0, ns, status.data()));
    }
    return ROBO_OK;
}

int32_t robo_gp_loglik_batch(robo_gp* g, const double* thetas, int32_t S, double mean_c, double* out_loglik,
                             int32_t* out_status) {
    if (!g || !thetas || S < 0 || !out_loglik) return ROBO_BAD_ARGUMENT;
    if (!g->has_data) {
        set_error("robo_gp_loglik_batch before robo_gp_set_data");
        return ROBO_NOT_FITTED;
    }
    if (S == 0) return ROBO_OK;
    g->fitted = false;   // the GP's own factor is not touched, but the call documents "unfitted after"
    return fit_batch_core(g, thetas, S, mean_c, out_loglik, out_status, nullptr);
}

// The whole ensemble chain on the device (mcmc.hip): no upload, synchronisation or host arithmetic between two half-steps.
int32_t robo_gp_mcmc_run(robo_gp* g, double mean_c, int32_t prior_kind, const double* prior_par, int32_t n_walkers,
                         int32_t n_steps, double a, const double* u_stretch, const int32_t* partner,
                         const double* u_accept, int32_t eval_start, double* pos, double* lnp, double* out_chain,
                         double* out_lnprob, int64_t* out_accepted) {
    if (!g || !pos || !lnp || n_walkers < 2 || (n_walkers & 1) || n_steps < 0 || !(a > 1.0)) return ROBO_BAD_ARGUMENT;
    if (n_steps > 0 && (!u_stretch || !partner || !u_accept)) return ROBO_BAD_ARGUMENT;
    if (prior_kind != 0 && ((prior_kind != 1 && prior_kind != 2) || !prior_par)) {
        set_error("robo_gp_mcmc_run: prior kind %d (0 = none, 1 = DefaultPrior, 2 = EnvPrior)", prior_kind);
        return ROBO_BAD_ARGUMENT;
    }
    if (prior_kind == 2) {
        const int P_ = robo_theta_size(g ? g->kind : 0, g ? g->dim : 1);
        const double n_ls = prior_par[5], n_lr = prior_par[6];
        if (!(n_ls >= 0 && n_lr >= 0 && n_ls == (double)(int)n_ls && n_lr == (double)(int)n_lr &&
              1 + (int)n_ls + (int)n_lr <= P_ - 1) || !(prior_par[8] > 0.0)) {
            set_error("robo_gp_mcmc_run: EnvPrior with n_ls=%g n_lr=%g sigma=%g does not fit %d hyper-parameters", n_ls,
                      n_lr, prior_par[8], P_);
            return ROBO_BAD_ARGUMENT;
        }
    }
    if (!g->has_data) {
        set_error("robo_gp_mcmc_run before robo_gp_set_data");
        return ROBO_NOT_FITTED;
    }
    robo_ctx* c = g->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    const int k = n_walkers, half = k / 2, D = g->dim, P = robo_theta_size(g->kind, D);
    const size_t np = (size_t)g->n_pad;
    {   // half an ensemble must fit the batch workspace in one pass (at the sizes of an MCMC fit it always does)
        const size_t per = np * np * sizeof(double) + np * (NB + (size_t)D) * sizeof(double);
        if ((size_t)half * per > workspace_bytes(c)) {
            set_error("robo_gp_mcmc_run: %d walkers of n_pad %zu exceed the batch workspace (ws_bytes)", half, np);
            return ROBO_BAD_SHAPE;
        }
    }
    g->fitted = false;
    ROBO_TRY(batch_ensure(g, half));
    // one scratch block: doubles first, then 64-bit counters, then ints
    const size_t nr = (size_t)n_steps * k;
    const size_t n_dbl = (size_t)k * P + k + (size_t)half * P + 2 * (size_t)half + 2 * nr + (size_t)k * n_steps * P + nr;
    const size_t bytes = n_dbl * sizeof(double) + (size_t)k * sizeof(long long) + (nr + 8) * sizeof(int);
    if (g->mcmc_bytes < bytes) {
        if (g->d_mcmc) ROBO_HIP_CHECK(hipFree(g->d_mcmc));
        g->d_mcmc = nullptr;
        g->mcmc_bytes = 0;
        ROBO_HIP_CHECK(hipMalloc((void**)&g->d_mcmc, bytes));
        g->mcmc_bytes = bytes;
    }
    McmcState st;
    memset(&st, 0, sizeof(st));
    double* d = reinterpret_cast<double*>(g->d_mcmc);
    st.d_pos = d; d += (size_t)k * P;
    st.d_lnp = d; d += k;
    st.d_q = d; d += (size_t)half * P;
    st.d_z = d; d += half;
    st.d_prior = d; d += half;
    double* d_uz = d; d += nr;
    double* d_ua = d; d += nr;
    st.d_chain = d; d += (size_t)k * n_steps * P;
    st.d_lnprob = d; d += nr;
    st.d_nacc = reinterpret_cast<long long*>(d);
    int* di = reinterpret_cast<int*>(st.d_nacc + k);   // [step counter, error flags, 6 spare | partners]
    st.d_it = di;
    st.d_err = di + 1;
    int* d_partner = di + 8;
    st.d_uz = d_uz; st.d_ua = d_ua; st.d_partner = d_partner;
    st.k = k; st.P = P; st.D = D; st.kind = g->kind; st.n = g->n; st.n_steps = n_steps; st.ns_eval = half;
    st.prior_kind = prior_kind; st.a = a; st.mean_c = mean_c;
    if (prior_kind != 0) for (int i = 0; i < (prior_kind == 2 ? 9 : 5); ++i) st.prior_par[i] = prior_par[i];
    st.d_sp = g->d_bsp; st.d_ism = g->d_bism; st.d_out = g->d_bout; st.d_fail = g->d_bfail;
    st.d_x2max = g->d_x2max;
    hipStream_t s = c->stream;
    ROBO_HIP_CHECK(hipMemcpyAsync(st.d_pos, pos, (size_t)k * P * sizeof(double), hipMemcpyHostToDevice, s));
    if (!eval_start) ROBO_HIP_CHECK(hipMemcpyAsync(st.d_lnp, lnp, (size_t)k * sizeof(double), hipMemcpyHostToDevice, s));
    if (nr > 0) {
        ROBO_HIP_CHECK(hipMemcpyAsync(d_uz, u_stretch, nr * sizeof(double), hipMemcpyHostToDevice, s));
        ROBO_HIP_CHECK(hipMemcpyAsync(d_ua, u_accept, nr * sizeof(double), hipMemcpyHostToDevice, s));
        ROBO_HIP_CHECK(hipMemcpyAsync(d_partner, partner, nr * sizeof(int), hipMemcpyHostToDevice, s));
    }
    ROBO_HIP_CHECK(hipMemsetAsync(st.d_nacc, 0, (size_t)k * sizeof(long long) + 8 * sizeof(int), s));
    FitBuffers fb;
    fb.K = g->d_bK; fb.k_stride = np * np;
    fb.prog = g->d_bprog;
    fb.Linv = g->d_bLinv; fb.linv_stride = np * NB;
    fb.Xs = g->d_bXs; fb.xs_stride = np * D;
    fb.sp = g->d_bsp;
    fb.fail = g->d_bfail;
    fb.out = g->d_bout;
    fb.ll_part = g->d_bllpart;
    fb.LinvP = nullptr;
    fb.host_out = nullptr;             // the likelihood terms are consumed on the device
    fb.gram_mixed = true;              // the proposals are formed on the device: each carries its own FitSample::direct
    fb.want_inverse = false;
    fb.skip_tail = c->tune.mcmc_fused_tail != 0 && g->n_pad > NB;     // (one-block factors reduce inside their diagonal kernel)
    fb.S = half;
    // one-block problems: the whole half-step in one launch (mcmc_block.hip mcmc_block_step_kernel; tuning: 0 never,
    // 1 only below 64 points, 2 or more = default: every one-block problem)
    const int bs = c->tune.mcmc_block_step;
    const bool one_block = (bs >= 2 ? g->n_pad == NB : (bs == 1 && g->n + 1 <= 64)) && !g->fp32_gram &&
                           g->kind != ROBO_KERNEL_FABOLAS;
    auto half_step = [&](int start, int first, int h, int it) -> int {
        if (one_block) return launch_mcmc_block_step(g, st, start, first, h, it);
        ROBO_TRY(launch_mcmc_propose_scale(c, st, start, first, h, it, g->d_X, g->d_bXs, g->n, g->n_pad, np * D));
        ROBO_TRY(launch_potrf(g, fb, true));        // gram + factorisation
        if (fb.skip_tail) {                          // likelihood terms + accept test + chain record: one launch
            const int nbk = g->n_pad / NB, nbf = (g->n % NB == 0 && nbk > 1) ? nbk - 1 : nbk;
            return launch_mcmc_tail(c, st, start, first, h, it, g->d_bK, np * np, g->n_pad, nbf, g->d_bfail);
        }
        return launch_mcmc_accept(c, st, start, first, h, it);
    };
    if (eval_start) {
        ROBO_TRY(half_step(1, 0, 0, 0));
        ROBO_TRY(half_step(1, half, 0, 0));
    }
    for (int it = 0; it < n_steps; ++it) {
        ROBO_TRY(half_step(0, 0, 0, it));
        ROBO_TRY(half_step(0, 0, 1, it));
    }
    int herr[2] = {0, 0};
    std::vector<long long> hacc((size_t)k);
    ROBO_HIP_CHECK(hipMemcpyAsync(pos, st.d_pos, (size_t)k * P * sizeof(double), hipMemcpyDeviceToHost, s));
    ROBO_HIP_CHECK(hipMemcpyAsync(lnp, st.d_lnp, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out_chain && nr > 0)
        ROBO_HIP_CHECK(hipMemcpyAsync(out_chain, st.d_chain, (size_t)k * n_steps * P * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out_lnprob && nr > 0)
        ROBO_HIP_CHECK(hipMemcpyAsync(out_lnprob, st.d_lnprob, nr * sizeof(double), hipMemcpyDeviceToHost, s));
    ROBO_HIP_CHECK(hipMemcpyAsync(hacc.data(), st.d_nacc, (size_t)k * sizeof(long long), hipMemcpyDeviceToHost, s));
    ROBO_HIP_CHECK(hipMemcpyAsync(herr, st.d_it, sizeof(herr), hipMemcpyDeviceToHost, s));
    ROBO_HIP_CHECK(hipStreamSynchronize(s));
    if (out_accepted) for (int w = 0; w < k; ++w) out_accepted[w] = (int64_t)hacc[(size_t)w];
    if (herr[1] & 1) {
        set_error("lnprob returned NaN.");
        return ROBO_BAD_ARGUMENT;
    }
    if (herr[1] & 2) {
        set_error("The initial lnprob was +inf.");
        return ROBO_BAD_ARGUMENT;
    }
    if (herr[1] & 4) {
        set_error("factorisation hand-off timed out inside the chain (tuning potrf_batch_follow=0 selects the launch-per-phase form)");
        return ROBO_RUNTIME_ERROR;
    }
    return ROBO_OK;
}

int32_t robo_gp_fit_batch(robo_gp* const* gps, int32_t S, const double* thetas, double mean_c, double* out_loglik,
                          int32_t* out_status) {
    if (!gps || !thetas || S < 0 || !out_loglik || !out_status) return ROBO_BAD_ARGUMENT;
    if (S == 0) return ROBO_OK;
    robo_gp* g0 = gps[0];
    if (!g0) return ROBO_BAD_ARGUMENT;
    if (!g0->has_data) {
        set_error("robo_gp_fit_batch: gps[0] has no data (robo_gp_set_data)");
        return ROBO_NOT_FITTED;
    }
    robo_ctx* c = g0->ctx;
    const int D = g0->dim, n = g0->n;
    for (int s = 0; s < S; ++s) {
        robo_gp* g = gps[s];
        if (!g || g->ctx != c || g->kind != g0->kind || g->dim != D || g->n_max < n) {
            set_error("robo_gp_fit_batch: gps[%d] must share context, kernel kind and dim with gps[0] and hold n=%d rows",
                      s, n);
            return ROBO_BAD_SHAPE;
        }
        for (int t = 0; t < s; ++t)
            if (gps[t] == g) {
                set_error("robo_gp_fit_batch: gps[%d] and gps[%d] are the same handle", t, s);
                return ROBO_BAD_ARGUMENT;
            }
        g->fitted = false;
    }
    const int P = robo_theta_size(g0->kind, D);
    auto keep = [&](int s0, int ns, const int* status) -> int {
        const double* hout = reinterpret_cast<const double*>(reinterpret_cast<const FitSample*>(g0->h_bstage) + g0->b_cap) +
                             (size_t)g0->b_cap * D;      // the batch's [ns][5] result block (fit_batch_core)
        // every kept factor goes to its handle in ONE launch (fit_keep.hip batch_keep_kernel)
        std::vector<KeepDst> dst((size_t)ns);
        for (int s = 0; s < ns; ++s) {
            KeepDst& d = dst[(size_t)s];
            memset(&d, 0, sizeof(d));
            if (status[s] != ROBO_OK) continue;
            robo_gp* g = gps[s0 + s];
            d.ok = 1;
            d.K = g->d_K; d.Linv = g->d_Linv; d.LinvP = g->d_LinvP; d.Xs = g->d_Xs; d.theta = g->d_theta; d.sp = g->d_sp;
            if (g != g0) {   // every handle ends up self-contained: same training data as gps[0]
                d.X = g->d_X;
                d.y = g->d_y;
            }
        }
        ROBO_HIP_CHECK(hipMemcpyAsync(g0->d_bkeep, dst.data(), (size_t)ns * sizeof(KeepDst), hipMemcpyHostToDevice, c->stream));
        ROBO_TRY(launch_batch_keep(g0, reinterpret_cast<const KeepDst*>(g0->d_bkeep), ns));
        for (int s = 0; s < ns; ++s) {
            if (status[s] != ROBO_OK) continue;
            robo_gp* g = gps[s0 + s];
            g->diag_min = hout[5 * s + 3];
            g->diag_max = hout[5 * s + 4];
            if (g != g0) {
                g->n = n;
                g->n_pad = g0->n_pad;
                g->has_data = true;
                g->fp32_gram = g0->fp32_gram;
                memcpy(g->x2max, g0->x2max, sizeof(g->x2max));
                ROBO_HIP_CHECK(hipMemcpyAsync(g->d_x2max, g->x2max, (size_t)D * sizeof(double), hipMemcpyHostToDevice, c->stream));
            }
            FitSample sp;
            double ism[MAX_DIM];
            ROBO_TRY(theta_to_sample(g, thetas + (size_t)(s0 + s) * P, mean_c, &sp, ism));
            g->cov = sp.cov;
            g->amp = sp.cov.amp;
            g->noise = sp.noise;
            g->mean_c = mean_c;
            g->loglik = out_loglik[s0 + s];
            g->fitted = true;
            g->fit_gen = next_fit_gen();
        }
        ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));
        return ROBO_OK;
    };
    return fit_batch_core(g0, thetas, S, mean_c, out_loglik, out_status, keep);
}

int32_t robo_gp_get_factor(robo_gp* g, double* out_L) {
    if (!g || !out_L) return ROBO_BAD_ARGUMENT;
    if (!g->fitted) return ROBO_NOT_FITTED;
    ROBO_HIP_CHECK(hipSetDevice(g->ctx->device));     // (a process may drive several devices: multi.hip)
    const size_t np = (size_t)g->n_pad;
    std::vector<double> h(np * np);
    ROBO_HIP_CHECK(hipMemcpyAsync(h.data(), g->d_K, np * np * sizeof(double), hipMemcpyDeviceToHost, g->ctx->stream));
    ROBO_HIP_CHECK(hipStreamSynchronize(g->ctx->stream));
    for (int i = 0; i < g->n; ++i)
        for (int j = 0; j < g->n; ++j) out_L[(size_t)i * g->n + j] = j <= i ? h[(size_t)i * np + j] : 0.0;
    return ROBO_OK;
}

int32_t robo_gp_get_gram(robo_gp* g, const double* theta, double* out_K) {
    if (!g || !theta || !out_K) return ROBO_BAD_ARGUMENT;
    if (!g->has_data) return ROBO_NOT_FITTED;
    g->fitted = false;   // d_K is overwritten
    ROBO_TRY(gp_build_gram(g, theta, 0.0));
    const size_t np = (size_t)g->n_pad;
    std::vector<double> h(np * np);
    ROBO_HIP_CHECK(hipMemcpyAsync(h.data(), g->d_K, np * np * sizeof(double), hipMemcpyDeviceToHost, g->ctx->stream));
    ROBO_HIP_CHECK(hipStreamSynchronize(g->ctx->stream));
    for (int i = 0; i < g->n; ++i)
        for (int j = 0; j < g->n; ++j)
            out_K[(size_t)i * g->n + j] = j <= i ? h[(size_t)i * np + j] : h[(size_t)j * np + i];
    return ROBO_OK;
}

}  // extern "C"
