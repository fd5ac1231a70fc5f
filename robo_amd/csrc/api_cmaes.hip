// C ABI of librobo_hip.so: the CMA-ES maximiser of a closed-form acquisition (robo_acq_cmaes_cand,
// robo_acq_cmaes_marginal_cand; the rule is stated in include/robo_hip.h).  Host-side orchestration only: every number is
// produced by the kernels in acq.hip / refine.hip (sweep, selection), cmaes.hip and the posterior's own.
//
//   sweep (acq.hip, unchanged)  ->  select_*: the R best candidates (refine.hip)  ->  cma_init_kernel
//   ->  T x [ cma_ask_kernel, per model predict_scaled on its kept handle, cma_tell_kernel ]  ->  cma_result_kernel
//
// Nothing between the sweep and the read-back touches the host.
#include <cmath>
#include <vector>

#include "api_internal.h"

namespace robo {

// Hansen's constants for n = D and lambda, positive weights only (w: mu entries)
static void cma_constants(int n, int lambda, CmaState* st, std::vector<double>* w) {
    const int mu = lambda / 2;
    w->resize((size_t)mu);
    double sum = 0.0, sum2 = 0.0;
    for (int i = 0; i < mu; ++i) {
        (*w)[i] = std::log((lambda + 1) / 2.0) - std::log((double)(i + 1));
        sum += (*w)[i];
    }
    for (int i = 0; i < mu; ++i) {
        (*w)[i] /= sum;
        sum2 += (*w)[i] * (*w)[i];
    }
    const double me = 1.0 / sum2, dn = (double)n;
    st->mu = mu;
    st->mueff = me;
    st->cs = (me + 2.0) / (dn + me + 5.0);
    st->ds = 1.0 + 2.0 * std::fmax(0.0, std::sqrt((me - 1.0) / (dn + 1.0)) - 1.0) + st->cs;
    st->cc = (4.0 + me / dn) / (dn + 4.0 + 2.0 * me / dn);
    st->c1 = 2.0 / ((dn + 1.3) * (dn + 1.3) + me);
    st->cmu = std::fmin(1.0 - st->c1, 2.0 * (me - 2.0 + 1.0 / me) / ((dn + 2.0) * (dn + 2.0) + me));
    st->chin = std::sqrt(dn) * (1.0 - 1.0 / (4.0 * dn) + 1.0 / (21.0 * dn * dn));
    st->log1mcs = std::log1p(-st->cs);
}

// marginal: the sweep is robo_acq_eval_marginal_cand's (accumulate, divide); otherwise robo_acq_eval_cand's
static int cma_core(robo_gp* const* gps, int32_t S, bool marginal, int32_t acq_kind, double par, const double* etas,
                    robo_cand* k, int32_t n_instances, int32_t lambda, int32_t n_generations, double sigma0, double sigma_min,
                    int32_t eig_every, const double* z, uint64_t seed, double* out_x, double* out_value,
                    int32_t* out_instance, uint32_t* out_flags, double* out_trace) {
    if (!gps || S < 1 || !etas || !k || !out_x) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(check_acq_kind(acq_kind));
    for (int s = 0; s < S; ++s)
        if (!gps[s]) return ROBO_BAD_ARGUMENT;
    robo_gp* g0 = gps[0];
    robo_ctx* c = g0->ctx;
    const int R = n_instances, L = lambda, T = n_generations, D = g0->dim;
    if (D < 2 || D > CMA_MAX) {
        set_error("cmaes: dim %d outside 2 .. %d (CMA-ES does not work in a one-dimensional space)", D, CMA_MAX);
        return ROBO_BAD_ARGUMENT;
    }
    if (L < 4 || L > CMA_MAX || R < 1 || R > CMA_MAX || T < 0 || eig_every < 0 || !(sigma0 > 0.0) || !std::isfinite(sigma0) ||
        !(sigma_min >= 0.0)) {
        set_error("cmaes: lambda %d (4 .. %d), n_instances %d (1 .. %d), n_generations %d (>= 0), eig_every %d (>= 0), "
                  "sigma0 %g (> 0, finite), sigma_min %g (>= 0)", L, CMA_MAX, R, CMA_MAX, T, eig_every, sigma0, sigma_min);
        return ROBO_BAD_ARGUMENT;
    }
    ROBO_TRY(ensemble_check("cmaes", 0, gps, S, k));
    for (int s = 0; s < S; ++s) {
        if (gps[s]->kind == ROBO_KERNEL_FABOLAS) {
            set_error("cmaes: sample %d has a Fabolas kernel, whose fidelity column is not a box coordinate", s);
            return ROBO_BAD_ARGUMENT;
        }
        for (int t = 0; t < s; ++t)
            if (gps[t] == gps[s]) {
                set_error("cmaes: samples %d and %d share a model handle (one posterior per handle)", t, s);
                return ROBO_BAD_ARGUMENT;
            }
    }
    const int64_t rows = (int64_t)R * L, m_pad = round_up64(rows, NB);
    if ((size_t)m_pad * g0->n_pad * sizeof(double) > workspace_bytes(c)) {
        set_error("cmaes: %d rows of %d columns exceed the solve workspace (ws_bytes)", (int)m_pad, g0->n_pad);
        return ROBO_BAD_SHAPE;
    }

    CmaState st;
    memset(&st, 0, sizeof(st));
    std::vector<double> w;
    cma_constants(D, L, &st, &w);
    st.R = R;
    st.D = D;
    st.L = L;
    st.T = T;
    st.S = S;
    st.kind = acq_kind;
    st.par = par;
    st.sigma0 = sigma0;
    st.sigma_min = sigma_min;
    st.seed = seed;
    st.m_pad = m_pad;
    const int auto_every = (int)std::floor(1.0 / (10.0 * D * (st.c1 + st.cmu)));
    st.eig_every = eig_every > 0 ? eig_every : (auto_every > 1 ? auto_every : 1);

    // The solve follows the library's rule for a batch of R lambda points (decide_winv): decided, W built and the workspaces
    // sized before the first generation -- nothing below waits for the device.
    std::vector<robo_cand*> hs((size_t)S);
    std::vector<char> use_w((size_t)S, 0);
    std::vector<CmaModel> models((size_t)S);
    for (int s = 0; T > 0 && s < S; ++s) {
        robo_gp* g = gps[s];
        ROBO_TRY(host_cand_rows(g, rows, &hs[s]));
        ROBO_TRY(cand_ensure_workspace(hs[s], g->n_pad, false));
        bool use = false;
        ROBO_TRY(decide_winv(g, hs[s], &use));
        use_w[s] = use ? 1 : 0;
        models[s] = CmaModel{g->d_theta, hs[s]->d_Xcs, hs[s]->d_mean, hs[s]->d_var, etas[s]};
    }

    if (!g0->cma) {
        g0->cma = new CmaWork();
        memset(g0->cma, 0, sizeof(CmaWork));
    }
    CmaWork* wk = g0->cma;
    if (wk->sel && (wk->sel->K != R || wk->sel->D != D)) {
        ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));
        refine_free(wk->sel);
        wk->sel = nullptr;
    }
    if (!wk->sel) ROBO_TRY(refine_alloc(c, R, D, &wk->sel));
    // one block: doubles first, then the model records, then the 4-byte words
    const size_t rd = (size_t)R * D, rdd = rd * D, nz = z ? (size_t)T * R * L * D : 0;
    BlockLayout lay(16);
    lay.add(&st.m, rd);
    lay.add(&st.sigma, (size_t)R);
    lay.add(&st.ps, rd);
    lay.add(&st.pc, rd);
    lay.add(&st.C, rdd);
    lay.add(&st.A, rdd);
    lay.add(&st.Ainv, rdd);
    lay.add(&st.bestx, rd);
    lay.add(&st.bestf, (size_t)R);
    lay.add(&st.x, rd * L);
    lay.add(&st.y, rd * L);
    lay.add(&st.out, (size_t)D + 3);
    lay.add(&st.w, w.size());
    lay.add(&st.z, nz);
    lay.add(&st.model, (size_t)S);
    lay.add(&st.gen, (size_t)R);
    lay.add(&st.frozen, (size_t)R);
    lay.add(&st.flags, 1);
    ROBO_TRY(dev_grow(c->stream, &wk->d_block, &wk->bytes, lay.bytes()));
    lay.bind(wk->d_block);
    if (!z) st.z = nullptr;
    const size_t trace_len = (size_t)(T + 1) * R * cma_trace_row(D, L);
    if (out_trace) ROBO_TRY(dev_grow(c->stream, &wk->d_trace, &wk->trace_cap, trace_len));
    st.trace = out_trace ? wk->d_trace : nullptr;

    // (w, z and model are const in CmaState, the kernels only read them: the uploads cast that away)
    const hipMemcpyKind h2d = hipMemcpyHostToDevice;
    ROBO_HIP_CHECK(hipMemcpyAsync((void*)st.w, w.data(), w.size() * sizeof(double), h2d, c->stream));
    if (nz > 0) ROBO_HIP_CHECK(hipMemcpyAsync((void*)st.z, z, nz * sizeof(double), h2d, c->stream));
    if (T > 0) ROBO_HIP_CHECK(hipMemcpyAsync((void*)st.model, models.data(), (size_t)S * sizeof(CmaModel), h2d, c->stream));

    ROBO_TRY(acq_sweep(gps, S, marginal, acq_kind, par, etas, k));
    // starts, generations, winner: launches only
    const RefineState& sel = wk->sel->st;
    int status = launch_refine_select(c, sel, k->d_acq, k->m, k->d_Xc, 0.0);
    if (status == ROBO_OK) status = launch_cma_init(c, st, sel);
    for (int g = 0; status == ROBO_OK && g < T; ++g) {
        status = launch_cma_ask(c, st, g);
        for (int s = 0; status == ROBO_OK && s < S; ++s) status = predict_scaled(gps[s], hs[s], use_w[s] != 0);
        if (status == ROBO_OK) status = launch_cma_tell(c, st, g);
    }
    if (status == ROBO_OK) status = launch_cma_result(c, st, k->d_flags);
    // read-back: the one synchronisation of the call
    std::vector<double> h((size_t)D + 3);
    ROBO_TRY(finish_call(k, "cmaes", status, {{h.data(), st.out, h.size() * sizeof(double)},
                                               {out_trace, wk->d_trace, trace_len * sizeof(double)}}));
    memcpy(out_x, h.data(), (size_t)D * sizeof(double));
    if (out_value) *out_value = h[D];
    long long v;
    memcpy(&v, &h[D + 1], sizeof(v));
    if (out_instance) *out_instance = (int32_t)v;
    memcpy(&v, &h[D + 2], sizeof(v));
    if (out_flags) *out_flags = (uint32_t)v;
    return ROBO_OK;
}

}  // namespace robo

using namespace robo;

extern "C" {

int32_t robo_acq_cmaes_cand(robo_gp* gp, int32_t acq_kind, double par, double eta, robo_cand* cand, int32_t n_instances,
                            int32_t lambda, int32_t n_generations, double sigma0, double sigma_min, int32_t eig_every,
                            const double* z, uint64_t seed, double* out_x, double* out_value, int32_t* out_instance,
                            uint32_t* out_flags, double* out_trace) {
    return cma_core(&gp, gp ? 1 : 0, false, acq_kind, par, &eta, cand, n_instances, lambda, n_generations, sigma0, sigma_min,
                    eig_every, z, seed, out_x, out_value, out_instance, out_flags, out_trace);
}

int32_t robo_acq_cmaes_marginal_cand(robo_gp* const* gps, int32_t S, int32_t acq_kind, double par, const double* etas,
                                     robo_cand* cand, int32_t n_instances, int32_t lambda, int32_t n_generations,
                                     double sigma0, double sigma_min, int32_t eig_every, const double* z, uint64_t seed,
                                     double* out_x, double* out_value, int32_t* out_instance, uint32_t* out_flags,
                                     double* out_trace) {
    return cma_core(gps, S, true, acq_kind, par, etas, cand, n_instances, lambda, n_generations, sigma0, sigma_min, eig_every,
                    z, seed, out_x, out_value, out_instance, out_flags, out_trace);
}

}  // extern "C"
