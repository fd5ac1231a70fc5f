// C ABI of librobo_hip.so, part 3: candidate handles and the posterior (mean, variance, gradients, covariance, the
// GP-MCMC mixture).  Host-side orchestration only: every number is produced by the kernels in predict.hip / winv.hip /
// predgrad.hip / acq.hip.
#include <functional>
#include <vector>

#include "api_internal.h"

namespace robo {

int cand_alloc(robo_ctx* ctx, int64_t m, int32_t dim, robo_cand** out) {
    if (!ctx || !out) return ROBO_BAD_ARGUMENT;
    if (m < 1 || dim < 1 || dim > MAX_DIM) {
        set_error("bad candidate shape m=%lld dim=%d", (long long)m, dim);
        return ROBO_BAD_SHAPE;
    }
    ROBO_HIP_CHECK(hipSetDevice(ctx->device));
    robo_cand* k = new robo_cand();
    memset(k, 0, sizeof(*k));
    k->ctx = ctx;
    k->dim = dim;
    k->m = m;
    k->m_pad = round_up64(m, NB);
    const size_t mp = (size_t)k->m_pad;
    ROBO_TRY(dev_alloc(&k->d_Xc, mp * dim));
    ROBO_TRY(dev_alloc(&k->d_Xcs, mp * dim));
    ROBO_TRY(dev_alloc(&k->d_q, mp));
    ROBO_TRY(dev_alloc(&k->d_mu, mp));
    ROBO_TRY(dev_alloc(&k->d_mean, mp));
    ROBO_TRY(dev_alloc(&k->d_var, mp));
    ROBO_TRY(dev_alloc(&k->d_acq, mp));
    ROBO_TRY(dev_alloc(&k->d_acq_sum, mp));
    k->n_part = (int)((m + 255) / 256);
    ROBO_TRY(dev_alloc(&k->d_part_val, (size_t)k->n_part + 1));
    ROBO_TRY(dev_alloc(&k->d_part_idx, (size_t)k->n_part + 1));
    ROBO_TRY(dev_alloc(&k->d_flags, 4));
    ROBO_HIP_CHECK(hipMemset(k->d_flags, 0, 4 * sizeof(unsigned)));   // cleared again by every read-back
    ctx_retain(ctx);
    *out = k;
    return ROBO_OK;
}

// size the (chunk x n_pad) solve workspace for this GP; grows, never shrinks
int cand_ensure_workspace(robo_cand* k, int n_pad, bool single_chunk) {
    const size_t row = (size_t)n_pad * sizeof(double);
    int64_t chunk = (int64_t)(workspace_bytes(k->ctx) / row) / NB * NB;
    if (chunk < NB) chunk = NB;
    if (chunk > k->m_pad || single_chunk) chunk = k->m_pad;
    const size_t need = (size_t)chunk * row;
    if (need > k->v_bytes) {
        if (k->d_V) ROBO_HIP_CHECK(hipFree(k->d_V));
        k->d_V = nullptr;
        k->v_bytes = 0;
        ROBO_HIP_CHECK(hipMalloc((void**)&k->d_V, need));
        k->v_bytes = need;
    }
    k->chunk = chunk;
    k->ldv = n_pad;
    return ROBO_OK;
}

// K4 + K5: fills cand->d_mean / d_var (asynchronous).  after_chunk(c0, cn), if given, runs while
// the chunk's V = L^-1 K*^T is still in the workspace (cross-covariances for entropy search).
// Small batches on a well-conditioned factor go through the explicit inverse W = L^-1 (winv.hip): one triangular
// product instead of n / 128 dependent block-row launches.  W's forward error is ~eps cond(L) where the substitution's
// is ~eps cond of a 128-block, so the path is taken only while cond_inf(L) = |L|_inf |W|_inf -- EXACT, two row-sum
// reductions when W is built (winv_ensure) -- stays below winv_cond_max (default 1e5: the measured error of the mean through W is <= ~10 eps cond, i.e.
// <= 1.1e-10 = the stated absolute tolerance of the mean; tests/parity_checks.py check_winv_guard_sweep); beyond it the
// substitution stays.  The diagonal ratio
// max L_ii / min L_ii <= cond_2(L) is only the cheap pre-filter that avoids building a W that would be rejected.
// the factor-side half of the decision (everything but the batch size): shared by winv_candidate and
// robo_gp_prefetch_inverse, so that a prefetch is launched exactly for the factors a small batch would use W on.
// min_blocks: 3 for a handful of candidates (matrix-vector form), winv_min_blocks otherwise
static bool winv_factor_ok(const robo_gp* g, int min_blocks) {
    const Tuning& t = g->ctx->tune;
    if (g->fp32_gram || t.predict_stepwise || t.winv_max <= 0) return false;
    if ((g->n + NB - 1) / NB < min_blocks) return false;
    return g->diag_min > 0.0 && g->diag_max <= (double)t.winv_cond_max * g->diag_min;
}

static int winv_min_blocks_for(const robo_gp* g, long long m) {
    const Tuning& t = g->ctx->tune;
    // a handful of candidates (the matrix-vector form, winv.hip) pays from three block rows on: N = 300 0.044 vs 0.065 ms,
    // N = 500 0.053 vs 0.086 ms against the 32-candidate substitution (r04x); larger batches from winv_min_blocks on
    return (m <= 8 && t.winv_gemv != 0 && t.winv_min_blocks > 3) ? 3 : t.winv_min_blocks;
}

bool winv_candidate(const robo_gp* g, const robo_cand* k) {
    if (k->m_pad > g->ctx->tune.winv_max) return false;
    return winv_factor_ok(g, winv_min_blocks_for(g, k->m));
}

int decide_winv(robo_gp* g, const robo_cand* k, bool* use) {
    *use = false;
    if (!winv_candidate(g, k)) return ROBO_OK;
    ROBO_TRY(winv_ensure(g));                  // builds W for this factor if needed and measures cond_inf(L)
    *use = g->winv_cond > 0.0 && g->winv_cond <= (double)g->ctx->tune.winv_cond_max;
    return ROBO_OK;
}

// need_v: the caller consumes V = L^-1 K_*^T itself (cross-covariances, full covariance), not only its reductions
int predict_core(robo_gp* g, robo_cand* k, bool single_chunk, const std::function<int(int64_t, int64_t)>& after_chunk,
                 bool need_v, bool allow_chain) {
    if (!g || !k) return ROBO_BAD_ARGUMENT;
    if (!g->fitted) {
        set_error("Model has to be trained first!");
        return ROBO_NOT_FITTED;
    }
    if (k->dim != g->dim || k->ctx != g->ctx) {
        set_error("candidate batch (dim %d) does not match the GP (dim %d) or lives on another context", k->dim,
                  g->dim);
        return ROBO_BAD_SHAPE;
    }
    ROBO_HIP_CHECK(hipSetDevice(g->ctx->device));
    k->solved_gen = 0;
    ROBO_TRY(cand_ensure_workspace(k, g->n_pad, single_chunk));
    bool winv = false;
    ROBO_TRY(decide_winv(g, k, &winv));
    ROBO_TRY(launch_scale_inputs(g->ctx, k->d_Xc, k->d_Xcs, g->d_theta, k->m, k->m_pad, g->dim));
    return predict_scaled(g, k, winv, after_chunk, need_v, false, allow_chain);
}

int predict_scaled(robo_gp* g, robo_cand* k, bool winv, const std::function<int(int64_t, int64_t)>& after_chunk, bool need_v,
                   bool events, bool allow_chain) {
    k->solved_gen = 0;
    // event slots 24..27 bracket the phases of the LAST chunk (bench.py reads them after a sync):
    //   24 -> 25 cross-gram, 25 -> 26 triangular solve (the MFMA kernel), 26 -> 27 post
    // (for small batches only when the phase events are switched on: phase_events_on)
    const bool ev = events || phase_events_on(g->ctx, k);
    for (int64_t c0 = 0; c0 < k->m_pad; c0 += k->chunk) {
        const int64_t cn = k->m_pad - c0 < k->chunk ? k->m_pad - c0 : k->chunk;
        if (ev) ROBO_TRY(record_phase(g->ctx, EV_PREDICT_BEGIN));
        if (winv) {
            if (ev) ROBO_TRY(record_phase(g->ctx, EV_PREDICT_GRAM_END));
            ROBO_TRY(launch_predict_winv(g, k, c0, cn, need_v || (bool)after_chunk));
        } else if (g->fp32_gram || g->ctx->tune.predict_stepwise) {
            // mixed precision (fp32 covariance entries) keeps the two-pass form
            ROBO_TRY(launch_cross_gram(g, k, c0, cn));
            if (ev) ROBO_TRY(record_phase(g->ctx, EV_PREDICT_GRAM_END));
            ROBO_TRY(launch_trsm(g, k, c0, cn));
        } else {
            if (ev) ROBO_TRY(record_phase(g->ctx, EV_PREDICT_GRAM_END));
            // small batches on two or more block rows: one launch chained by hand-offs, where the caller looks at its
            // time-out word at the synchronisation it ends in (allow_chain)
            if (allow_chain && chain_wanted(g, cn)) ROBO_TRY(launch_predict_chain(g, k, c0, cn));
            else ROBO_TRY(launch_predict_fused(g, k, c0, cn));
        }
        if (ev) ROBO_TRY(record_phase(g->ctx, EV_PREDICT_SOLVE_END));
        if (after_chunk) ROBO_TRY(after_chunk(c0, cn));
    }
    if (!k->defer_post) ROBO_TRY(launch_post(g, k, 0, k->m_pad));
    if (ev) ROBO_TRY(record_phase(g->ctx, EV_PREDICT_END));
    return ROBO_OK;
}

// per-sample posteriors of S fitted GPs on one candidate handle -> rows 0 .. S - 1 of the handle's (>= cap) x m_pad
// sample tables d_mu_all / d_var_all (asynchronous)
int predict_samples(robo_gp* const* gps, int32_t S, robo_cand* k, int cap) {
    ROBO_HIP_CHECK(hipSetDevice(k->ctx->device));
    const size_t mp = (size_t)k->m_pad;
    if (cap < S) cap = S;
    if (k->s_cap < cap) {
        if (k->d_mu_all) ROBO_HIP_CHECK(hipFree(k->d_mu_all));
        if (k->d_var_all) ROBO_HIP_CHECK(hipFree(k->d_var_all));
        k->d_mu_all = k->d_var_all = nullptr;
        k->s_cap = 0;
        ROBO_TRY(dev_alloc(&k->d_mu_all, (size_t)cap * mp));
        ROBO_TRY(dev_alloc(&k->d_var_all, (size_t)cap * mp));
        k->s_cap = cap;
    }
    hipStream_t st = k->ctx->stream;
    for (int s = 0; s < S; ++s) {
        ROBO_TRY(predict_core(gps[s], k));
        ROBO_HIP_CHECK(hipMemcpyAsync(k->d_mu_all + (size_t)s * mp, k->d_mean, mp * sizeof(double), hipMemcpyDeviceToDevice, st));
        ROBO_HIP_CHECK(hipMemcpyAsync(k->d_var_all + (size_t)s * mp, k->d_var, mp * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    return ROBO_OK;
}

// The candidate handle behind the host-array entry points (robo_gp_predict, robo_acq_eval).  Small batches -- the
// reference's 500 random candidates per iteration, the 1 x D calls of its single-point maximisers -- come back with
// the same size over and over: their handle (a dozen device allocations) is kept with the GP and only re-uploaded
// (0.14 -> ~0.08 ms per call at N <= 100).  Larger batches are created and destroyed per call as before.
int host_cand(robo_gp* g, const double* Xc, int64_t m, robo_cand** out, bool* kept) {
    *kept = m <= 16384;
    if (!*kept) return robo_cand_create(g->ctx, Xc, m, g->dim, out);
    if (g->host_cand && g->host_cand->m == m) {
        ROBO_TRY(robo_cand_set_points(g->host_cand, Xc, m));
    } else {
        robo_cand_destroy(g->host_cand);
        g->host_cand = nullptr;
        ROBO_TRY(robo_cand_create(g->ctx, Xc, m, g->dim, &g->host_cand));
    }
    *out = g->host_cand;
    return ROBO_OK;
}

int host_cand_rows(robo_gp* g, int64_t m, robo_cand** out) {
    if (!(g->host_cand && g->host_cand->m == m)) {
        robo_cand_destroy(g->host_cand);
        g->host_cand = nullptr;
        ROBO_TRY(cand_alloc(g->ctx, m, g->dim, &g->host_cand));
    }
    g->host_cand->solved_gen = 0;
    *out = g->host_cand;
    return ROBO_OK;
}

}  // namespace robo

using namespace robo;

extern "C" {

int32_t robo_cand_create(robo_ctx* ctx, const double* Xc, int64_t m, int32_t dim, robo_cand** out) {
    if (!Xc) return ROBO_BAD_ARGUMENT;
    robo_cand* k = nullptr;
    ROBO_TRY(cand_alloc(ctx, m, dim, &k));
    ROBO_HIP_CHECK(hipMemcpyAsync(k->d_Xc, Xc, (size_t)m * dim * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ROBO_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    *out = k;
    return ROBO_OK;
}

int32_t robo_cand_set_points(robo_cand* k, const double* Xc, int64_t m) {
    if (!k || !Xc) return ROBO_BAD_ARGUMENT;
    if (m != k->m) {
        set_error("robo_cand_set_points: batch holds %lld points, got %lld", (long long)k->m, (long long)m);
        return ROBO_BAD_SHAPE;
    }
    ROBO_HIP_CHECK(hipSetDevice(k->ctx->device));
    k->solved_gen = 0;
    ROBO_HIP_CHECK(hipMemcpyAsync(k->d_Xc, Xc, (size_t)m * k->dim * sizeof(double), hipMemcpyHostToDevice, k->ctx->stream));
    ROBO_HIP_CHECK(hipStreamSynchronize(k->ctx->stream));   // the caller's buffer is only borrowed for the call
    return ROBO_OK;
}

int32_t robo_cand_create_uniform(robo_ctx* ctx, int64_t m, int32_t dim, uint64_t seed, robo_cand** out) {
    robo_cand* k = nullptr;
    ROBO_TRY(cand_alloc(ctx, m, dim, &k));
    ROBO_TRY(launch_uniform(ctx, k->d_Xc, m, k->m_pad, dim, seed));
    ROBO_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    *out = k;
    return ROBO_OK;
}

int32_t robo_cand_create_sobol(robo_ctx* ctx, int64_t m, int32_t dim, const uint64_t* sv, const uint64_t* shift,
                               int32_t bits, uint64_t first_index, robo_cand** out) {
    if (!sv || !shift || bits < 1 || bits > 64) return ROBO_BAD_ARGUMENT;
    if (bits < 64 && (first_index + (uint64_t)m) > (1ull << bits)) {
        set_error("Sobol: points %llu .. %llu exceed 2^%d", (unsigned long long)first_index,
                  (unsigned long long)(first_index + (uint64_t)m), bits);
        return ROBO_BAD_SHAPE;
    }
    robo_cand* k = nullptr;
    ROBO_TRY(cand_alloc(ctx, m, dim, &k));
    // the direction numbers (dim x bits) and the digital shift (dim) ride in the still unused scaled-candidate buffer
    if ((size_t)dim * bits + dim > (size_t)k->m_pad * dim) {
        robo_cand_destroy(k);
        set_error("Sobol: batch too small to stage the direction numbers (m_pad %lld < bits + 1)", (long long)k->m_pad);
        return ROBO_BAD_SHAPE;
    }
    unsigned long long* d_sv = reinterpret_cast<unsigned long long*>(k->d_Xcs);
    unsigned long long* d_shift = d_sv + (size_t)dim * bits;
    int st = ROBO_OK;
    hipError_t e = hipMemcpyAsync(d_sv, sv, (size_t)dim * bits * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_shift, shift, (size_t)dim * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) {
        set_error("Sobol: upload of the direction numbers failed: %s", hipGetErrorString(e));
        st = ROBO_RUNTIME_ERROR;
    }
    if (st == ROBO_OK) st = launch_sobol(ctx, k->d_Xc, m, k->m_pad, dim, d_sv, d_shift, bits, first_index);
    if (st == ROBO_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) st = ROBO_RUNTIME_ERROR;
    if (st != ROBO_OK) {
        robo_cand_destroy(k);
        return st;
    }
    *out = k;
    return ROBO_OK;
}

int32_t robo_cand_create_random(robo_ctx* ctx, int64_t m, int32_t dim, uint64_t seed, int64_t n_uniform,
                                const double* loc, const double* scale, robo_cand** out) {
    if (!loc || !scale || n_uniform < 0 || n_uniform > m) return ROBO_BAD_ARGUMENT;
    robo_cand* k = nullptr;
    ROBO_TRY(cand_alloc(ctx, m, dim, &k));
    // loc/scale ride in the (still unused) scaled-candidate buffer
    ROBO_HIP_CHECK(hipMemcpyAsync(k->d_Xcs, loc, (size_t)dim * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ROBO_HIP_CHECK(hipMemcpyAsync(k->d_Xcs + dim, scale, (size_t)dim * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ROBO_TRY(launch_random_candidates(ctx, k->d_Xc, k->m_pad, dim, seed, n_uniform, k->d_Xcs, k->d_Xcs + dim));
    ROBO_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    *out = k;
    return ROBO_OK;
}

int32_t robo_cand_get_point(robo_cand* k, int64_t index, double* out_x) {
    if (!k || !out_x) return ROBO_BAD_ARGUMENT;
    if (index < 0 || index >= k->m) {
        set_error("candidate index %lld outside [0, %lld)", (long long)index, (long long)k->m);
        return ROBO_BAD_SHAPE;
    }
    ROBO_HIP_CHECK(hipSetDevice(k->ctx->device));
    ROBO_HIP_CHECK(hipMemcpyAsync(out_x, k->d_Xc + (size_t)index * k->dim, (size_t)k->dim * sizeof(double),
                                  hipMemcpyDeviceToHost, k->ctx->stream));
    ROBO_HIP_CHECK(hipStreamSynchronize(k->ctx->stream));
    return ROBO_OK;
}

int32_t robo_cand_workspace_chunk(robo_cand* k, int64_t* out_chunk) {
    if (!k || !out_chunk) return ROBO_BAD_ARGUMENT;
    *out_chunk = k->chunk;
    return ROBO_OK;
}

int32_t robo_cand_last_solve_kernel(robo_cand* k, char* buf, int32_t buf_len) {
    if (!k || !buf || buf_len < 1) return ROBO_BAD_ARGUMENT;
    const int used = snprintf(buf, (size_t)buf_len, "%s", k->solve_kernel ? k->solve_kernel : "");
    // behind the terminator, where the buffer has room: the kernel of the last bounds pass of the acquisition screen
    if (used >= 0 && used + 1 < buf_len)
        snprintf(buf + used + 1, (size_t)(buf_len - used - 1), "%s", k->scr_bounds_kernel ? k->scr_bounds_kernel : "");
    return ROBO_OK;
}

int32_t robo_cand_get_points(robo_cand* k, double* out_Xc) {
    if (!k || !out_Xc) return ROBO_BAD_ARGUMENT;
    ROBO_HIP_CHECK(hipSetDevice(k->ctx->device));
    ROBO_HIP_CHECK(hipMemcpyAsync(out_Xc, k->d_Xc, (size_t)k->m * k->dim * sizeof(double), hipMemcpyDeviceToHost,
                                  k->ctx->stream));
    ROBO_HIP_CHECK(hipStreamSynchronize(k->ctx->stream));
    return ROBO_OK;
}

int32_t robo_cand_destroy(robo_cand* k) {
    if (!k) return ROBO_OK;
    hipSetDevice(k->ctx->device);
    hipStreamSynchronize(k->ctx->stream);
    hipFree(k->d_Xc);
    hipFree(k->d_Xcs);
    hipFree(k->d_V);
    hipFree(k->d_q);
    hipFree(k->d_mu);
    hipFree(k->d_mean);
    hipFree(k->d_var);
    hipFree(k->d_acq);
    hipFree(k->d_acq_sum);
    hipFree(k->d_mu_all);
    hipFree(k->d_var_all);
    hipFree(k->d_S);
    hipFree(k->d_F);
    hipFree(k->d_Q);
    hipFree(k->d_G);
    hipFree(k->d_igc);
    hipFree(k->d_kg);
    free(k->h_igkey);
    hipFree(k->d_Ks);
    hipFree(k->d_P);
    hipFree(k->d_qpart);
    hipFree(k->d_part_val);
    hipFree(k->d_part_idx);
    hipFree(k->d_flags);
    hipFree(k->d_scr_up);
    hipFree(k->d_scr_lo);
    hipFree(k->d_scr_cnt);
    hipFree(k->d_scr_map);
    hipFree(k->d_chain);
    robo_cand_destroy(k->scr_sub);
    refine_free(k->scr_probe);
    robo_ctx* ctx = k->ctx;
    delete k;
    ctx_release(ctx);
    return ROBO_OK;
}

int32_t robo_gp_prefetch_inverse(robo_gp* g) {
    if (!g) return ROBO_BAD_ARGUMENT;
    if (!g->fitted) {
        set_error("Model has to be trained first!");
        return ROBO_NOT_FITTED;
    }
    // the same conditions under which a small batch would ask for W (winv_candidate), for the smallest batch that could
    // come (a handful of candidates: from three block rows on)
    if (!winv_factor_ok(g, winv_min_blocks_for(g, 1))) return ROBO_OK;
    // only for handles that HAVE served a small batch through W before (its buffers exist): a model that is only ever asked
    // for large batches never pays the two n_pad^2 buffers or the build
    if (!g->d_Winv) return ROBO_OK;
    ROBO_HIP_CHECK(hipSetDevice(g->ctx->device));
    return winv_launch(g);
}

int32_t robo_gp_factor_cond(robo_gp* g, double* out) {
    if (!g || !out) return ROBO_BAD_ARGUMENT;
    if (!g->fitted) {
        set_error("Model has to be trained first!");
        return ROBO_NOT_FITTED;
    }
    ROBO_HIP_CHECK(hipSetDevice(g->ctx->device));
    ROBO_TRY(winv_ensure(g));
    out[0] = g->winv_cond;
    out[1] = g->diag_min;
    out[2] = g->diag_max;
    return ROBO_OK;
}

int32_t robo_gp_predict_cand(robo_gp* g, robo_cand* k, double* out_mean, double* out_var) {
    // the chained solve's time-out word is looked at behind the call's own synchronisation; a launch that gave up (it never
    // should) turns the chain off for the context, and the second pass runs the launches
    for (int pass = 0;; ++pass) {
        ROBO_TRY(predict_core(g, k, false, nullptr, false, true));
        hipStream_t st = g->ctx->stream;
        if (out_mean)
            ROBO_HIP_CHECK(hipMemcpyAsync(out_mean, k->d_mean, (size_t)k->m * sizeof(double), hipMemcpyDeviceToHost, st));
        if (out_var)
            ROBO_HIP_CHECK(hipMemcpyAsync(out_var, k->d_var, (size_t)k->m * sizeof(double), hipMemcpyDeviceToHost, st));
        ROBO_HIP_CHECK(hipStreamSynchronize(st));
        if (!chain_timed_out(g->ctx) || pass > 0) return ROBO_OK;
    }
}

int32_t robo_gp_predict_mixture_cand(robo_gp* const* gps, int32_t S, robo_cand* k, double* out_mean,
                                     double* out_var) {
    if (!gps || S < 1 || !k) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(predict_samples(gps, S, k, S));
    hipStream_t st = k->ctx->stream;
    ROBO_TRY(launch_mixture(k, S));
    if (out_mean)
        ROBO_HIP_CHECK(hipMemcpyAsync(out_mean, k->d_mean, (size_t)k->m * sizeof(double), hipMemcpyDeviceToHost, st));
    if (out_var)
        ROBO_HIP_CHECK(hipMemcpyAsync(out_var, k->d_var, (size_t)k->m * sizeof(double), hipMemcpyDeviceToHost, st));
    ROBO_HIP_CHECK(hipStreamSynchronize(st));
    return ROBO_OK;
}

int32_t robo_gp_predict(robo_gp* g, const double* Xc, int64_t m, double* out_mean, double* out_var) {
    if (!g) return ROBO_BAD_ARGUMENT;
    if (!g->fitted) {
        set_error("Model has to be trained first!");
        return ROBO_NOT_FITTED;
    }
    robo_cand* k = nullptr;
    bool kept = false;
    ROBO_TRY(host_cand(g, Xc, m, &k, &kept));
    const int st = robo_gp_predict_cand(g, k, out_mean, out_var);
    if (!kept) robo_cand_destroy(k);
    return st;
}

int32_t robo_gp_predict_grad(robo_gp* g, const double* Xc, int64_t m, double* out_mean, double* out_var,
                             double* out_dmean, double* out_dvar) {
    if (!g || !Xc || !out_dmean || !out_dvar) return ROBO_BAD_ARGUMENT;
    if (!g->fitted) {
        set_error("Model has to be trained first!");
        return ROBO_NOT_FITTED;
    }
    const int D = g->dim, E = D + 1;
    robo_ctx* c = g->ctx;
    hipStream_t st = c->stream;
    robo_cand* kc = nullptr;   // the real candidates (upload + scaling + output buffers)
    ROBO_TRY(robo_cand_create(c, Xc, m, D, &kc));
    // candidates per pass: D + 1 workspace rows each, rows padded to the 128-row solve tile
    const size_t row_bytes = (size_t)g->n_pad * sizeof(double);
    int64_t per = (int64_t)(workspace_bytes(c) / row_bytes / NB * NB) / E;
    if (per < 1) per = 1;
    if (per > m) per = m;
    // cross_grad_kernel and predgrad_post_kernel put (a multiple of) the candidate index on grid.y / grid.x
    if (per + NB > 65535) per = 65535 - NB;
    const int64_t rows_pad = round_up64(per * E, NB);
    robo_cand* ws = nullptr;   // the pseudo-row solve workspace
    double *d_dm = nullptr, *d_dv = nullptr;
    int status = cand_alloc(c, rows_pad, 1, &ws);
    if (status == ROBO_OK) status = cand_ensure_workspace(ws, g->n_pad, true);
    if (status == ROBO_OK) status = dev_alloc(&d_dm, (size_t)m * D);
    if (status == ROBO_OK) status = dev_alloc(&d_dv, (size_t)m * D);
    if (status == ROBO_OK) status = launch_scale_inputs(c, kc->d_Xc, kc->d_Xcs, g->d_theta, kc->m, kc->m_pad, D);
    for (int64_t c0 = 0; status == ROBO_OK && c0 < m; c0 += per) {
        const int64_t cn = m - c0 < per ? m - c0 : per;
        const int64_t rp = round_up64(cn * E, NB);
        status = launch_cross_grad(g, kc->d_Xcs, ws->d_V, c0, cn, rp);
        if (status == ROBO_OK) status = launch_trsm(g, ws, 0, rp);
        if (status == ROBO_OK)
            status = launch_predgrad_post(g, ws->d_V, ws->d_q, ws->d_mu, kc->d_Xcs, c0, cn, kc->d_mean, kc->d_var, d_dm, d_dv);
    }
    if (status == ROBO_OK) {
        hipError_t e = hipSuccess;
        if (out_mean) e = hipMemcpyAsync(out_mean, kc->d_mean, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out_var)
            e = hipMemcpyAsync(out_var, kc->d_var, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out_dmean, d_dm, (size_t)m * D * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out_dvar, d_dv, (size_t)m * D * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            set_error("robo_gp_predict_grad copy-out failed: %s", hipGetErrorString(e));
            status = ROBO_RUNTIME_ERROR;
        }
    } else {
        hipStreamSynchronize(st);
    }
    hipFree(d_dm);
    hipFree(d_dv);
    robo_cand_destroy(ws);
    robo_cand_destroy(kc);
    return status;
}

int32_t robo_gp_predict_cov(robo_gp* g, const double* Xc, int64_t m, double* out_mean, double* out_cov) {
    if (!g || !out_cov) return ROBO_BAD_ARGUMENT;
    if (!g->fitted) {
        set_error("Model has to be trained first!");
        return ROBO_NOT_FITTED;
    }
    if (m > 16384) {
        set_error("robo_gp_predict_cov is for small batches (m=%lld > 16384)", (long long)m);
        return ROBO_BAD_SHAPE;
    }
    robo_cand* k = nullptr;
    ROBO_TRY(robo_cand_create(g->ctx, Xc, m, g->dim, &k));
    double* d_cov = nullptr;
    int st = ROBO_OK;
    if (hipMalloc((void**)&d_cov, (size_t)m * m * sizeof(double)) != hipSuccess) {
        set_error("hipMalloc of the %lld x %lld covariance failed", (long long)m, (long long)m);
        st = ROBO_RUNTIME_ERROR;
    }
    for (int pass = 0; st == ROBO_OK; ++pass) {      // (the second pass: after a time-out of the chained solve, robo_gp_predict_cand)
        st = predict_core(g, k, true, nullptr, true, true);
        if (st == ROBO_OK) st = launch_cov(g, k, d_cov);
        if (st != ROBO_OK) break;
        hipStream_t s = g->ctx->stream;
        hipError_t e = hipMemcpyAsync(out_cov, d_cov, (size_t)m * m * sizeof(double), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && out_mean)
            e = hipMemcpyAsync(out_mean, k->d_mean, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            set_error("predict_cov copy-out failed: %s", hipGetErrorString(e));
            st = ROBO_RUNTIME_ERROR;
        }
        if (st != ROBO_OK || !chain_timed_out(g->ctx) || pass > 0) break;
    }
    if (d_cov) hipFree(d_cov);
    robo_cand_destroy(k);
    return st;
}

}  // extern "C"
