// C ABI of librobo_hip.so, part 5: the knowledge gradient over a discretisation (robo_kg_eval_cand,
// robo_kg_eval_marginal_cand, robo_kg_eval_moments; the rule is stated in include/robo_hip.h).  Host-side orchestration
// only: every number is produced by the kernels in predict.hip / infogain.hip / kg.hip / acq.hip.
#include <cmath>
#include <vector>

#include "api_internal.h"

namespace robo {
constexpr const char* KG_LABEL = "knowledge gradient";
constexpr int KG_MAX_DISC = 64;

static int kg_check(int64_t nb, const double* sn2s, int S) {
    if (nb < 1 || nb > KG_MAX_DISC) {
        set_error("%s: %lld discretisation points, must be in [1, %d]", KG_LABEL, (long long)nb, KG_MAX_DISC);
        return ROBO_BAD_ARGUMENT;
    }
    for (int s = 0; s < S; ++s)
        if (!(sn2s[s] >= 0.0)) {
            set_error("%s: sn2 = %g of sample %d is negative or NaN", KG_LABEL, sn2s[s], s);
            return ROBO_BAD_ARGUMENT;
        }
    return ROBO_OK;
}

// the covariance rows d_S (m_pad x NB, shared with entropy search) and [S x KG_MAX_DISC discretisation means |
// S x m x (nb + 2) trace] on the handle
static int kg_ensure(robo_cand* k, int S, size_t trace_len) {
    if (!k->d_S) ROBO_TRY(dev_alloc(&k->d_S, (size_t)k->m_pad * NB));
    return dev_grow(k->ctx->stream, &k->d_kg, &k->kg_cap, (size_t)S * KG_MAX_DISC + trace_len);
}

// sum over the samples of KG into k->d_acq_sum, the discretisation means and the trace into k->d_kg (asynchronous)
static int kg_accumulate(robo_gp* const* gps, int32_t S, robo_cand* k, robo_cand* rep, const double* sn2s,
                         int32_t include_self, bool want_trace) {
    const int nb = (int)rep->m;
    robo_ctx* c = k->ctx;
    double* d_trace = k->d_kg + (size_t)S * KG_MAX_DISC;
    // event slots 30 -> 31 bracket the KG kernel of the LAST sample
    const bool ev = phase_events_on(c, k);
    for (int s = 0; s < S; ++s) {
        robo_gp* g = gps[s];
        // the discretisation's solve is kept across calls while the factor and the points stay the same, as in ig_core
        if (!(rep->solved_gen != 0 && rep->solved_gp == g && rep->solved_gen == g->fit_gen)) {
            ROBO_TRY(predict_core(g, rep, true, nullptr, true));
            rep->solved_gp = g;
            rep->solved_gen = g->fit_gen;
        }
        double* d_disc = k->d_kg + (size_t)s * KG_MAX_DISC;
        ROBO_HIP_CHECK(hipMemcpyAsync(d_disc, rep->d_mean, (size_t)nb * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        ROBO_TRY(clear_flags_on_error(k, predict_core(g, k, false, [&](int64_t c0, int64_t cn) {
            return launch_cross_cov(g, k, rep, c0, cn, k->d_S, false);
        })));
        if (ev) ROBO_TRY(record_phase(c, EV_FOLD_BEGIN));
        ROBO_TRY(clear_flags_on_error(k, launch_kg(c, k->d_S, k->d_var, k->d_mean, d_disc, k->m, nb, sn2s[s], include_self, s == 0,
                                                   k->d_acq_sum, k->d_flags,
                                                   want_trace ? d_trace + (size_t)s * k->m * (nb + 2) : nullptr)));
        if (ev) ROBO_TRY(record_phase(c, EV_FOLD_END));
    }
    return ROBO_OK;
}

static int kg_core(robo_gp* const* gps, int32_t S, robo_cand* k, robo_cand* rep, const double* sn2s, int32_t include_self,
                   double* out_kg, double* out_max, int64_t* out_argmax, uint32_t* out_flags, double* out_disc_mean,
                   double* out_trace) {
    if (!gps || S < 1 || !k || !rep || !sn2s) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(kg_check(rep->m, sn2s, S));
    if (rep->ctx != k->ctx || rep->dim != k->dim || rep == k) {
        set_error("%s: the discretisation (dim %d) and the candidates (dim %d) must be two handles of one dimension on "
                  "one context", KG_LABEL, rep->dim, k->dim);
        return ROBO_BAD_SHAPE;
    }
    ROBO_TRY(ensemble_check(KG_LABEL, ENSEMBLE_ONE_KIND_FP64, gps, S, k));
    const int nb = (int)rep->m;
    const size_t trace_len = out_trace ? (size_t)S * k->m * (nb + 2) : 0;
    ROBO_TRY(kg_ensure(k, S, trace_len));
    ROBO_TRY(kg_accumulate(gps, S, k, rep, sn2s, include_self, out_trace != nullptr));
    ROBO_TRY(clear_flags_on_error(k, launch_argmax(k, k->d_acq_sum, (double)S)));
    hipStream_t st = k->ctx->stream;
    if (out_disc_mean)
        for (int s = 0; s < S; ++s)
            if (hipMemcpyAsync(out_disc_mean + (size_t)s * nb, k->d_kg + (size_t)s * KG_MAX_DISC, (size_t)nb * sizeof(double),
                               hipMemcpyDeviceToHost, st) != hipSuccess)
                return finish_call(k, KG_LABEL, ROBO_RUNTIME_ERROR, {});
    ROBO_TRY(finish_call(k, KG_LABEL, ROBO_OK,
                         {{out_trace, k->d_kg + (size_t)S * KG_MAX_DISC, trace_len * sizeof(double)}}, false));
    // (max, argmax, flags) [+ the values] and the one synchronisation of the call
    return clear_flags_on_error(k, acq_read_back(k, k->d_acq, out_kg, out_max, out_argmax, out_flags));
}

}  // namespace robo

using namespace robo;

extern "C" {

int32_t robo_kg_eval_cand(robo_gp* g, robo_cand* k, robo_cand* rep, double sn2, int32_t include_self, double* out_kg,
                          double* out_max, int64_t* out_argmax, uint32_t* out_flags, double* out_disc_mean,
                          double* out_trace) {
    return kg_core(&g, g ? 1 : 0, k, rep, &sn2, include_self, out_kg, out_max, out_argmax, out_flags, out_disc_mean,
                   out_trace);
}

int32_t robo_kg_eval_marginal_cand(robo_gp* const* gps, int32_t S, robo_cand* k, robo_cand* rep, const double* sn2s,
                                   int32_t include_self, double* out_kg, double* out_max, int64_t* out_argmax,
                                   uint32_t* out_flags, double* out_disc_mean, double* out_trace) {
    return kg_core(gps, S, k, rep, sn2s, include_self, out_kg, out_max, out_argmax, out_flags, out_disc_mean, out_trace);
}

int32_t robo_kg_eval_moments(robo_ctx* ctx, int64_t m, int32_t nb, double sn2, int32_t include_self, const double* s,
                             const double* v, const double* mean, const double* disc_mean, double* out_kg,
                             double* out_max, int64_t* out_argmax, uint32_t* out_flags) {
    if (!ctx || !s || !v || !mean || !disc_mean) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(kg_check(nb, &sn2, 1));
    robo_cand* k = nullptr;
    ROBO_TRY(moments_handle(ctx, mean, v, m, "knowledge gradient: upload of the moments", &k));
    int st = kg_ensure(k, 1, 0);
    if (st == ROBO_OK) {
        std::vector<double> hs((size_t)k->m_pad * NB, 0.0);
        for (int64_t c = 0; c < m; ++c)
            for (int b = 0; b < nb; ++b) hs[(size_t)c * NB + b] = s[c * nb + b];
        // (synchronised: the staging vector dies with this scope)
        st = upload_rows(ctx, "knowledge gradient: upload of the covariances",
                         {{k->d_S, hs.data(), hs.size()}, {k->d_kg, disc_mean, (size_t)nb}}, true);
    }
    if (st == ROBO_OK)
        st = launch_kg(ctx, k->d_S, k->d_var, k->d_mean, k->d_kg, m, nb, sn2, include_self, true, k->d_acq_sum, k->d_flags,
                       nullptr);
    return moments_finish(k, st, true, out_kg, out_max, out_argmax, out_flags);
}

}  // extern "C"
