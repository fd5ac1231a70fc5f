// C ABI of librobo_hip.so, part 4: the closed-form acquisitions over a candidate batch, entropy search's information
// gain, and the plumbing every ensemble driver shares (refine.hip, batch.hip, mes.hip, comm.hip, multi.hip).  Host-side
// orchestration only: every number is produced by the kernels in predict.hip / acq.hip / infogain.hip / igmc.hip.
#include <cmath>
#include <functional>
#include <vector>

#include "api_internal.h"

namespace robo {

int check_acq_kind(int kind) {
    if (kind < ROBO_ACQ_EI || kind > ROBO_ACQ_LCB) {
        set_error("unknown acquisition kind %d", kind);
        return ROBO_BAD_ARGUMENT;
    }
    return ROBO_OK;
}

// The flag word of a candidate handle is OR-ed into by the acquisition kernels and cleared by the read-back's report
// kernel.  An error return between the two (a later sample's posterior failing, a launch failure) would leave stale
// ZERO_SIGMA / NEGATIVE_EI bits in a handle that lives on (kept host-array handles, representer points): clear them.
int clear_flags_on_error(robo_cand* k, int status) {
    if (status != ROBO_OK && k && k->d_flags) hipMemsetAsync(k->d_flags, 0, 4 * sizeof(unsigned), k->ctx->stream);
    return status;
}

// D2H of (max, argmax, flags) [+ the acquisition vector] and the one synchronisation of the call
int acq_read_back(robo_cand* k, const double* d_vec, double* out_vec, double* out_max, int64_t* out_argmax,
                         uint32_t* out_flags) {
    robo_ctx* c = k->ctx;
    double* hp = c->h_pinned;
    // (max, argmax, flags) -> pinned memory; clears the flag word (the screen's fused tail has done both already)
    if (!k->best_reported) ROBO_TRY(launch_report_best(k, hp));
    k->best_reported = false;
    if (out_vec)
        ROBO_HIP_CHECK(hipMemcpyAsync(out_vec, d_vec, (size_t)k->m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (out_max) *out_max = hp[0];
    if (out_argmax) {
        long long i;
        memcpy(&i, hp + 1, sizeof(i));
        *out_argmax = (int64_t)i;
    }
    if (out_flags) {
        unsigned f;
        memcpy(&f, hp + 2, sizeof(f));
        *out_flags = f;
    }
    return ROBO_OK;
}

int acq_accumulate(robo_gp* const* gps, int32_t S, int32_t acq_kind, double par, const double* etas, robo_cand* k,
                   bool allow_chain) {
    if (!gps || S < 1 || !k || !etas) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(check_acq_kind(acq_kind));
    ROBO_HIP_CHECK(hipSetDevice(k->ctx->device));
    for (int s = 0; s < S; ++s) {
        ROBO_TRY(clear_flags_on_error(k, predict_core(gps[s], k, false, nullptr, false, allow_chain)));
        ROBO_TRY(clear_flags_on_error(k, launch_acq(k->ctx, k, acq_kind, par, etas[s], true, s == 0)));
    }
    return ROBO_OK;
}

int acq_sweep(robo_gp* const* gps, int32_t S, bool marginal, int32_t acq_kind, double par, const double* etas, robo_cand* k,
              bool allow_chain) {
    if (marginal) {
        ROBO_TRY(acq_accumulate(gps, S, acq_kind, par, etas, k, allow_chain));
        return clear_flags_on_error(k, launch_argmax(k, k->d_acq_sum, (double)S));
    }
    ROBO_TRY(check_acq_kind(acq_kind));
    ROBO_TRY(predict_core(gps[0], k, false, nullptr, false, allow_chain));
    return clear_flags_on_error(k, launch_acq(gps[0]->ctx, k, acq_kind, par, etas[0], false, false));
}

int ensemble_check(const char* label, unsigned flags, robo_gp* const* gps, int32_t S, const robo_cand* k) {
    const bool mes = flags & ENSEMBLE_MES_VERDICTS, strict = flags & ENSEMBLE_ONE_KIND_FP64;
    for (int s = 0; s < S; ++s) {
        const robo_gp* g = gps[s];
        if (!g) return ROBO_BAD_ARGUMENT;
        if (!g->fitted) {
            if (mes) set_error("%s: sample %d has no fitted model (Model has to be trained first!)", label, s);
            else set_error("Model has to be trained first!");
            return mes ? ROBO_BAD_ARGUMENT : ROBO_NOT_FITTED;
        }
        if (mes) continue;
        if (g->dim != k->dim || g->ctx != k->ctx || g->n != gps[0]->n || (strict && g->kind != gps[0]->kind)) {
            set_error("%s: sample %d (dim %d, n %d) does not match the candidates (dim %d), the first sample (n %d) or "
                      "their context", label, s, g->dim, g->n, k->dim, gps[0]->n);
            return ROBO_BAD_SHAPE;
        }
        if (strict && g->fp32_gram) {
            set_error("%s needs fp64 covariance entries (robo_gp_set_precision 0)", label);
            return ROBO_BAD_ARGUMENT;
        }
    }
    ROBO_HIP_CHECK(hipSetDevice(gps[0]->ctx->device));
    return ROBO_OK;
}

int finish_call(robo_cand* k, const char* label, int status, std::initializer_list<ReadBack> copies, bool sync) {
    hipStream_t st = k->ctx->stream;
    hipError_t e = hipSuccess;
    if (status == ROBO_OK) {
        for (const ReadBack& c : copies)
            if (e == hipSuccess && c.dst) e = hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && sync) e = hipStreamSynchronize(st);
        if (e == hipSuccess) return ROBO_OK;
        set_error("%s: read-back failed: %s", label, hipGetErrorString(e));
        status = ROBO_RUNTIME_ERROR;
    }
    hipStreamSynchronize(st);
    return clear_flags_on_error(k, status);
}

int moments_handle(robo_ctx* ctx, const double* mean, const double* var, int64_t m, const char* what, robo_cand** out) {
    robo_cand* k = nullptr;
    ROBO_TRY(cand_alloc(ctx, m, 1, &k));
    hipError_t e = hipMemcpyAsync(k->d_mean, mean, (size_t)m * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(k->d_var, var, (size_t)m * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) {
        set_error("%s failed: %s", what, hipGetErrorString(e));
        robo_cand_destroy(k);            // (waits for the stream)
        return ROBO_RUNTIME_ERROR;
    }
    *out = k;
    return ROBO_OK;
}

int upload_rows(robo_ctx* ctx, const char* what, std::initializer_list<UploadRows> rows, bool sync) {
    hipError_t e = hipSuccess;
    for (const UploadRows& r : rows)
        if (e == hipSuccess && r.count > 0)
            e = hipMemcpyAsync(r.dst, r.src, r.count * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && sync) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) return ROBO_OK;
    set_error("%s failed: %s", what, hipGetErrorString(e));
    return ROBO_RUNTIME_ERROR;
}

int moments_finish(robo_cand* k, int status, bool reduce, double* out_vec, double* out_max, int64_t* out_argmax,
                   uint32_t* out_flags) {
    if (status == ROBO_OK && reduce) status = launch_argmax(k, k->d_acq_sum, 1.0);
    if (status == ROBO_OK) status = acq_read_back(k, k->d_acq, out_vec, out_max, out_argmax, out_flags);
    else hipStreamSynchronize(k->ctx->stream);
    robo_cand_destroy(k);
    return status;
}

int models_check(const char* label, const char* the_models, robo_gp* const* gps, int32_t S, const robo_cand* k,
                 const std::function<void(int)>& shape_error) {
    if (!gps || S < 1 || !k) return ROBO_BAD_ARGUMENT;
    for (int s = 0; s < S; ++s)
        if (!gps[s]) return ROBO_BAD_ARGUMENT;
    for (int s = 0; s < S; ++s)
        if (gps[s]->ctx != k->ctx) {
            set_error("%s: %s and the candidates must live on one context", label, the_models);
            return ROBO_BAD_ARGUMENT;
        }
    for (int s = 0; s < S; ++s)
        if (gps[s]->dim != k->dim) {
            shape_error(s);
            return ROBO_BAD_SHAPE;
        }
    for (int s = 0; s < S; ++s)
        if (!gps[s]->fitted) {
            set_error("Model has to be trained first!");
            return ROBO_NOT_FITTED;
        }
    ROBO_HIP_CHECK(hipSetDevice(k->ctx->device));
    return ROBO_OK;
}

int models_fold_launch(robo_gp* const* gps, int32_t S, robo_cand* k, int slot_begin, const std::function<int()>& fold) {
    robo_ctx* c = k->ctx;
    // the S sweeps, each chunked by the workspace
    ROBO_TRY(clear_flags_on_error(k, predict_samples(gps, S, k, S)));
    const bool ev = phase_events_on(c, k);
    if (ev) ROBO_TRY(record_phase(c, slot_begin));
    ROBO_TRY(clear_flags_on_error(k, fold()));
    if (ev) ROBO_TRY(record_phase(c, slot_begin + 1));
    return clear_flags_on_error(k, launch_argmax(k, k->d_acq_sum, 1.0));
}

int models_fold(const char* label, robo_gp* const* gps, int32_t S, robo_cand* k, int slot_begin,
                const std::function<int()>& fold, ReadBack trace, double* out_vec, double* out_max, int64_t* out_argmax,
                uint32_t* out_flags) {
    ROBO_TRY(models_fold_launch(gps, S, k, slot_begin, fold));
    ROBO_TRY(finish_call(k, label, ROBO_OK, {trace}, false));
    // (max, argmax, flags) [+ the values] and the one synchronisation of the call
    return clear_flags_on_error(k, acq_read_back(k, k->d_acq, out_vec, out_max, out_argmax, out_flags));
}

// ---------------------------------------------------------------------------------------
// entropy search: information gain of a candidate batch
// ---------------------------------------------------------------------------------------
static int ig_ensure(robo_cand* k, int kf) {
    const size_t mp = (size_t)k->m_pad;
    if (!k->d_S) ROBO_TRY(dev_alloc(&k->d_S, mp * NB));
    const size_t need_f = (size_t)k->chunk * kf;
    if (k->f_cap < need_f) {
        hipFree(k->d_F);
        k->d_F = nullptr;
        k->f_cap = 0;
        ROBO_TRY(dev_alloc(&k->d_F, need_f));
        k->f_cap = need_f;
    }
    if (k->q_cap < (size_t)k->chunk) {
        hipFree(k->d_Q);
        k->d_Q = nullptr;
        ROBO_TRY(dev_alloc(&k->d_Q, (size_t)k->chunk * NB));
        k->q_cap = (size_t)k->chunk;
    }
    if (k->g_cap < (size_t)kf) {
        hipFree(k->d_G);
        hipFree(k->d_igc);
        k->d_G = k->d_igc = nullptr;
        if (k->h_igkey) k->h_igkey[0] = -1.0;      // the device copies are gone: no cached EP state
        ROBO_TRY(dev_alloc(&k->d_G, (size_t)NB * kf));
        ROBO_TRY(dev_alloc(&k->d_igc, (size_t)128 + 512 + 64 * 64));
        k->g_cap = (size_t)kf;
    }
    return ROBO_OK;
}

// upload the EP state: consts = [logP (64) | lmb (64) | W (npts) | dlogPdMu (nb x nb)], G (128 x kf)
static int ig_upload(robo_cand* k, int nb, int npts, int kf, const double* logP, const double* lmb, const double* W,
                     const double* dlogPdMu, const double* dlogPdSigma, const double* dlogPdMudMu) {
    // The EP state changes once per update() of the acquisition function and is then evaluated on batch after batch:
    // the 2.5 MB re-layout + upload + synchronisation below is skipped when all six arrays equal, bit for bit, the
    // ones this handle's device copies were made from (0.1 ms of memcmp instead of ~0.5 ms per call at Nb = 50).
    const int ntri_k = nb * (nb + 1) / 2;
    const size_t lens[6] = {(size_t)nb, (size_t)nb, (size_t)npts, (size_t)nb * nb, (size_t)nb * ntri_k,
                            (size_t)nb * nb * nb};
    const double* srcs[6] = {logP, lmb, W, dlogPdMu, dlogPdSigma, dlogPdMudMu};
    size_t total = 2;
    for (size_t l : lens) total += l;
    if (k->h_igkey && k->igkey_len == total && k->h_igkey[0] == (double)nb && k->h_igkey[1] == (double)npts) {
        bool same = true;
        size_t off = 2;
        for (int a = 0; a < 6 && same; ++a) {
            same = memcmp(k->h_igkey + off, srcs[a], lens[a] * sizeof(double)) == 0;
            off += lens[a];
        }
        if (same) return ROBO_OK;
    }
    if (k->igkey_len != total) {
        free(k->h_igkey);
        k->h_igkey = (double*)malloc(total * sizeof(double));
        k->igkey_len = k->h_igkey ? total : 0;
    }
    if (k->h_igkey) {
        k->h_igkey[0] = -1.0;      // invalid until the upload below has been issued
        size_t off = 2;
        for (int a = 0; a < 6; ++a) {
            memcpy(k->h_igkey + off, srcs[a], lens[a] * sizeof(double));
            off += lens[a];
        }
    }
    std::vector<double> hc((size_t)128 + npts + (size_t)nb * nb, 0.0), hg((size_t)NB * kf, 0.0);
    for (int i = 0; i < nb; ++i) {
        hc[i] = logP[i];
        hc[64 + i] = lmb[i];
    }
    for (int p = 0; p < npts; ++p) hc[128 + p] = W[p];
    for (int i = 0; i < nb * nb; ++i) hc[128 + npts + i] = dlogPdMu[i];
    const int ntri = nb * (nb + 1) / 2;
    for (int i = 0; i < nb; ++i) {
        double* g1 = hg.data() + (size_t)i * kf;            // q1_i = s^T dlogPdMudMu_i s
        double* g2 = hg.data() + (size_t)(64 + i) * kf;     // q2_i = sum_{a>=b} dlogPdSigma_i[ab] s_a s_b
        for (int e = 0; e < nb * nb; ++e) g1[e] = dlogPdMudMu[(size_t)i * nb * nb + e];
        int idx = 0;
        for (int a = 0; a < nb; ++a)
            for (int b = 0; b <= a; ++b) g2[a * nb + b] = dlogPdSigma[(size_t)i * ntri + idx++];
    }
    hipStream_t st = k->ctx->stream;
    ROBO_HIP_CHECK(hipMemcpyAsync(k->d_igc, hc.data(), hc.size() * sizeof(double), hipMemcpyHostToDevice, st));
    ROBO_HIP_CHECK(hipMemcpyAsync(k->d_G, hg.data(), hg.size() * sizeof(double), hipMemcpyHostToDevice, st));
    ROBO_HIP_CHECK(hipStreamSynchronize(st));   // the staging vectors die with this scope
    if (k->h_igkey) {
        k->h_igkey[0] = (double)nb;
        k->h_igkey[1] = (double)npts;
    }
    return ROBO_OK;
}

static int ig_check(int nb, int npts) {
    if (nb < 2 || nb > 64 || npts < 1 || npts > 512) {
        set_error("information gain: Nb=%d must be in [2, 64], Np=%d in [1, 512]", nb, npts);
        return ROBO_BAD_SHAPE;
    }
    return ROBO_OK;
}

static double ig_entropy(int nb, const double* logP, const double* lmb) {
    double H = 0.0;
    for (int i = 0; i < nb; ++i) H -= std::exp(logP[i]) * (logP[i] + lmb[i]);
    return H;
}

// dH of every candidate of k into k->d_acq_sum (asynchronous)
static int ig_core(robo_gp* g, robo_cand* k, robo_cand* rep, int32_t npts, double sn2, const double* logP,
                   const double* lmb, const double* W, const double* dlogPdMu, const double* dlogPdSigma,
                   const double* dlogPdMudMu) {
    if (!g || !k || !rep || !logP || !lmb || !W || !dlogPdMu || !dlogPdSigma || !dlogPdMudMu) return ROBO_BAD_ARGUMENT;
    const int nb = (int)rep->m;
    ROBO_TRY(ig_check(nb, npts));
    const int kf = round_up(nb * nb, 16);
    // V of the representer points: kept across calls while the factor and the points stay the same (the reference
    // does its representer-point work once per update(), information_gain.py:127-167, not per compute())
    if (!(rep->solved_gen != 0 && rep->solved_gp == g && rep->solved_gen == g->fit_gen)) {
        ROBO_TRY(predict_core(g, rep, true, nullptr, true));
        rep->solved_gp = g;
        rep->solved_gen = g->fit_gen;
    }
    ROBO_TRY(cand_ensure_workspace(k, g->n_pad, false));
    ROBO_TRY(ig_ensure(k, kf));
    ROBO_TRY(ig_upload(k, nb, npts, kf, logP, lmb, W, dlogPdMu, dlogPdSigma, dlogPdMudMu));
    ROBO_TRY(predict_core(g, k, false, [&](int64_t c0, int64_t cn) { return launch_cross_cov(g, k, rep, c0, cn, k->d_S); }));
    const double H = ig_entropy(nb, logP, lmb);
    for (int64_t c0 = 0; c0 < k->m_pad; c0 += k->chunk) {
        const int64_t cn = k->m_pad - c0 < k->chunk ? k->m_pad - c0 : k->chunk;
        ROBO_TRY(launch_ig_dh(g->ctx, k->d_S, k->d_var, k->d_F, k->d_Q, k->d_G, k->d_igc, c0, cn, k->m, nb, npts, kf,
                              sn2, H, k->d_acq_sum));
    }
    return ROBO_OK;
}

// dH / (exp(log-cost mean) + overhead) of every candidate into k->d_acq (and the best of them into the argmax slots):
// the local half of robo_ig_eval_per_cost_cand and of its sharded form (comm.hip)
int ig_per_cost_core(robo_gp* g, robo_cand* k, robo_cand* rep, int32_t npts, double sn2, const double* logP,
                            const double* lmb, const double* W, const double* dlogPdMu, const double* dlogPdSigma,
                            const double* dlogPdMudMu, robo_gp* cost_gp, robo_cand* cost_k, double overhead) {
    if (!cost_gp || !cost_k || !k) return ROBO_BAD_ARGUMENT;
    if (cost_k->m != k->m || cost_k->ctx != k->ctx || cost_gp->ctx != k->ctx || cost_k == k) {
        set_error("information gain per unit cost: the cost model's candidate handle must hold the same %lld candidates "
                  "(in the cost model's input space) on the same context", (long long)k->m);
        return ROBO_BAD_SHAPE;
    }
    ROBO_TRY(ig_core(g, k, rep, npts, sn2, logP, lmb, W, dlogPdMu, dlogPdSigma, dlogPdMudMu));
    ROBO_TRY(predict_core(cost_gp, cost_k));                  // cost_k->d_mean: the cost model's (log-cost) mean
    ROBO_TRY(launch_per_cost(k->ctx, k->d_acq_sum, cost_k->d_mean, overhead, k->m));
    return launch_argmax(k, k->d_acq_sum, 1.0);
}

}  // namespace robo

using namespace robo;

extern "C" {

int32_t robo_acq_eval_cand(robo_gp* g, int32_t acq_kind, double par, double eta, robo_cand* k, double* out_acq,
                           double* out_max, int64_t* out_argmax, uint32_t* out_flags) {
    // the chained solve's time-out word is looked at behind the read-back's synchronisation: a launch that gave up (it never
    // should) turns the chain off for the context, and the second pass runs the launches
    for (int pass = 0;; ++pass) {
        int st = acq_sweep_best(g, acq_kind, par, eta, k, out_acq != nullptr, true, k->ctx->h_pinned);
        if (st == ROBO_CHAIN_RETRY && pass == 0) continue;
        ROBO_TRY(st);
        st = acq_read_back(k, k->d_acq, out_acq, out_max, out_argmax, out_flags);
        if (st == ROBO_OK && chain_timed_out(k->ctx) && pass == 0) continue;
        return clear_flags_on_error(k, st);
    }
}

int32_t robo_acq_eval(robo_gp* g, int32_t acq_kind, double par, double eta, const double* Xc, int64_t m,
                      double* out_acq, double* out_max, int64_t* out_argmax, uint32_t* out_flags) {
    if (!g) return ROBO_BAD_ARGUMENT;
    if (!g->fitted) {
        set_error("Model has to be trained first!");
        return ROBO_NOT_FITTED;
    }
    robo_cand* k = nullptr;
    bool kept = false;
    ROBO_TRY(host_cand(g, Xc, m, &k, &kept));
    const int st = robo_acq_eval_cand(g, acq_kind, par, eta, k, out_acq, out_max, out_argmax, out_flags);
    if (!kept) robo_cand_destroy(k);
    return st;
}

int32_t robo_acq_eval_marginal_cand(robo_gp* const* gps, int32_t S, int32_t acq_kind, double par, const double* etas,
                                    robo_cand* k, double* out_acq, double* out_max, int64_t* out_argmax,
                                    uint32_t* out_flags) {
    for (int pass = 0;; ++pass) {          // (the second pass: after a time-out of the chained solve, robo_acq_eval_cand)
        ROBO_TRY(acq_sweep(gps, S, true, acq_kind, par, etas, k, true));
        const int st = acq_read_back(k, k->d_acq, out_acq, out_max, out_argmax, out_flags);
        if (st == ROBO_OK && chain_timed_out(k->ctx) && pass == 0) continue;
        return clear_flags_on_error(k, st);
    }
}

int32_t robo_acq_eval_sum_cand(robo_gp* const* gps, int32_t S, int32_t acq_kind, double par, const double* etas,
                               robo_cand* k, double* out_acq_sum, uint32_t* out_flags) {
    ROBO_TRY(acq_accumulate(gps, S, acq_kind, par, etas, k));
    ROBO_TRY(clear_flags_on_error(k, launch_argmax(k, k->d_acq_sum, 1.0)));
    return clear_flags_on_error(k, acq_read_back(k, k->d_acq_sum, out_acq_sum, nullptr, nullptr, out_flags));
}

int32_t robo_acq_eval_moments(robo_ctx* ctx, int32_t acq_kind, double par, double eta, const double* mean,
                              const double* var, int64_t m, double* out_acq, double* out_max, int64_t* out_argmax,
                              uint32_t* out_flags) {
    if (!ctx || !mean || !var) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(check_acq_kind(acq_kind));
    robo_cand* k = nullptr;
    ROBO_TRY(moments_handle(ctx, mean, var, m, "robo_acq_eval_moments upload", &k));
    return moments_finish(k, launch_acq(ctx, k, acq_kind, par, eta, false, false), false, out_acq, out_max, out_argmax,
                          out_flags);
}

int32_t robo_gp_cross_cov(robo_gp* g, robo_cand* k, robo_cand* rep, double* out_cov) {
    if (!g || !k || !rep || !out_cov) return ROBO_BAD_ARGUMENT;
    if (rep->m > 64) {
        set_error("cross-covariance reference set limited to 64 points (got %lld)", (long long)rep->m);
        return ROBO_BAD_SHAPE;
    }
    ROBO_TRY(predict_core(g, rep, true, nullptr, true));
    ROBO_TRY(cand_ensure_workspace(k, g->n_pad, false));
    ROBO_TRY(ig_ensure(k, 16));
    ROBO_TRY(predict_core(g, k, false, [&](int64_t c0, int64_t cn) { return launch_cross_cov(g, k, rep, c0, cn, k->d_S); }));
    std::vector<double> h((size_t)k->m * NB);
    ROBO_HIP_CHECK(hipMemcpyAsync(h.data(), k->d_S, h.size() * sizeof(double), hipMemcpyDeviceToHost, g->ctx->stream));
    ROBO_HIP_CHECK(hipStreamSynchronize(g->ctx->stream));
    for (int64_t c = 0; c < k->m; ++c)
        for (int64_t b = 0; b < rep->m; ++b) out_cov[c * rep->m + b] = h[(size_t)c * NB + b];
    return ROBO_OK;
}

int32_t robo_ig_eval_cand(robo_gp* g, robo_cand* k, robo_cand* rep, int32_t npts, double sn2, const double* logP,
                          const double* lmb, const double* W, const double* dlogPdMu, const double* dlogPdSigma,
                          const double* dlogPdMudMu, double* out_dh, double* out_max, int64_t* out_argmax) {
    ROBO_TRY(ig_core(g, k, rep, npts, sn2, logP, lmb, W, dlogPdMu, dlogPdSigma, dlogPdMudMu));
    ROBO_TRY(launch_argmax(k, k->d_acq_sum, 1.0));
    return acq_read_back(k, k->d_acq, out_dh, out_max, out_argmax, nullptr);
}

int32_t robo_ig_eval_per_cost_cand(robo_gp* g, robo_cand* k, robo_cand* rep, int32_t npts, double sn2, const double* logP,
                                   const double* lmb, const double* W, const double* dlogPdMu, const double* dlogPdSigma,
                                   const double* dlogPdMudMu, robo_gp* cost_gp, robo_cand* cost_k, double overhead,
                                   double* out_values, double* out_max, int64_t* out_argmax) {
    ROBO_TRY(ig_per_cost_core(g, k, rep, npts, sn2, logP, lmb, W, dlogPdMu, dlogPdSigma, dlogPdMudMu, cost_gp, cost_k,
                              overhead));
    return acq_read_back(k, k->d_acq, out_values, out_max, out_argmax, nullptr);
}

int32_t robo_ig_eval_moments(robo_ctx* ctx, int64_t m, int32_t nb, int32_t npts, double sn2, const double* s,
                             const double* v, const double* logP, const double* lmb, const double* W,
                             const double* dlogPdMu, const double* dlogPdSigma, const double* dlogPdMudMu,
                             double* out_dh) {
    if (!ctx || !s || !v || !out_dh) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(ig_check(nb, npts));
    const int kf = round_up(nb * nb, 16);
    robo_cand* k = nullptr;
    ROBO_TRY(cand_alloc(ctx, m, 1, &k));
    k->chunk = k->m_pad;
    int st = ig_ensure(k, kf);
    if (st == ROBO_OK) st = ig_upload(k, nb, npts, kf, logP, lmb, W, dlogPdMu, dlogPdSigma, dlogPdMudMu);
    if (st == ROBO_OK) {
        std::vector<double> hs((size_t)k->m_pad * NB, 0.0);
        for (int64_t c = 0; c < m; ++c)
            for (int b = 0; b < nb; ++b) hs[(size_t)c * NB + b] = s[c * nb + b];
        hipError_t e = hipMemcpyAsync(k->d_S, hs.data(), hs.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(k->d_var, v, (size_t)m * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            set_error("robo_ig_eval_moments upload failed: %s", hipGetErrorString(e));
            st = ROBO_RUNTIME_ERROR;
        }
    }
    if (st == ROBO_OK)
        st = launch_ig_dh(ctx, k->d_S, k->d_var, k->d_F, k->d_Q, k->d_G, k->d_igc, 0, k->m_pad, m, nb, npts, kf, sn2,
                          ig_entropy(nb, logP, lmb), k->d_acq_sum);
    if (st == ROBO_OK) {
        hipError_t e = hipMemcpyAsync(out_dh, k->d_acq_sum, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) st = ROBO_RUNTIME_ERROR;
    }
    robo_cand_destroy(k);
    return st;
}

int32_t robo_igmc_eval_cand(robo_gp* g, robo_cand* k, robo_cand* rep, int32_t n_outcomes, int32_t nf, double sn2,
                            const double* Mb, const double* Vb, const double* logP, const double* lmb, const double* W,
                            const double* z, double* out_dh, double* out_max, int64_t* out_argmax, uint32_t* out_flags) {
    if (!g || !k || !rep) return ROBO_BAD_ARGUMENT;
    if (rep->m < 1 || rep->m > 64) {
        set_error("Monte-Carlo information gain: %lld representer points, must be in [1, 64]", (long long)rep->m);
        return ROBO_BAD_ARGUMENT;
    }
    const int nb = (int)rep->m;
    // the representer points' solve is kept across calls, as in ig_core
    if (!(rep->solved_gen != 0 && rep->solved_gp == g && rep->solved_gen == g->fit_gen)) {
        ROBO_TRY(predict_core(g, rep, true, nullptr, true));
        rep->solved_gp = g;
        rep->solved_gen = g->fit_gen;
    }
    ROBO_TRY(cand_ensure_workspace(k, g->n_pad, false));
    ROBO_TRY(ig_ensure(k, 16));
    ROBO_TRY(predict_core(g, k, false, [&](int64_t c0, int64_t cn) { return launch_cross_cov(g, k, rep, c0, cn, k->d_S); }));
    ROBO_TRY(clear_flags_on_error(k, mc_eval_gains(g->ctx, k->m, nb, n_outcomes, nf, sn2, k->d_S, NB, k->d_var, Mb, Vb,
                                                   logP, lmb, W, z, k->d_acq_sum, nullptr, nullptr, k->d_flags)));
    ROBO_TRY(clear_flags_on_error(k, launch_argmax(k, k->d_acq_sum, 1.0)));
    return clear_flags_on_error(k, acq_read_back(k, k->d_acq, out_dh, out_max, out_argmax, out_flags));
}

}  // extern "C"
