// C ABI of librobo_hip.so: the differential-evolution maximiser of a closed-form acquisition (robo_acq_de_cand,
// robo_acq_de_marginal_cand; the rule is stated in include/robo_hip.h).  Host-side orchestration only: every number is produced
// by the kernels in acq.hip (sweep), de.hip and the posterior's own.
//
//   sweep (acq.hip, unchanged)  ->  T x [ de_step_kernel(g), per model predict_scaled on its kept handle ]
//   ->  de_step_kernel(T): the last select  ->  de_result_kernel
//
// Nothing between the sweep and the read-back touches the host.
#include <cmath>
#include <vector>

#include "api_internal.h"

namespace robo {

// marginal: the sweep is robo_acq_eval_marginal_cand's (accumulate, divide); otherwise robo_acq_eval_cand's
static int de_core(robo_gp* const* gps, int32_t S, bool marginal, int32_t acq_kind, double par, const double* etas, robo_cand* k,
                   int32_t n_instances, int32_t popsize, int32_t n_generations, double f_lo, double f_hi, double cr, double tol,
                   double atol, const double* u, uint64_t seed, double* out_x, double* out_value, int32_t* out_instance,
                   int32_t* out_generations, uint32_t* out_flags, double* out_trace) {
    if (!gps || S < 1 || !etas || !k || !out_x) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(check_acq_kind(acq_kind));
    for (int s = 0; s < S; ++s)
        if (!gps[s]) return ROBO_BAD_ARGUMENT;
    robo_gp* g0 = gps[0];
    robo_ctx* c = g0->ctx;
    const int R = n_instances, NP = popsize, T = n_generations, D = g0->dim;
    if (D < 1 || D > DE_MAX_DIM) {
        set_error("de: dim %d outside 1 .. %d", D, DE_MAX_DIM);
        return ROBO_BAD_ARGUMENT;
    }
    if (NP < 4 || NP > DE_MAX_NP || R < 1 || R > DE_MAX_R || NP * D > DE_MAX_POP || R * NP > 16384 || T < 0) {
        set_error("de: popsize %d (4 .. %d, popsize dim <= %d), n_instances %d (1 .. %d, n_instances popsize <= 16384), "
                  "n_generations %d (>= 0)", NP, DE_MAX_NP, DE_MAX_POP, R, DE_MAX_R, T);
        return ROBO_BAD_ARGUMENT;
    }
    if (!(0.0 <= f_lo && f_lo <= f_hi && f_hi <= 2.0) || !(cr >= 0.0 && cr <= 1.0) || !(tol >= 0.0) || !(atol >= 0.0)) {
        set_error("de: 0 <= f_lo %g <= f_hi %g <= 2, cr %g in [0, 1], tol %g and atol %g >= 0", f_lo, f_hi, cr, tol, atol);
        return ROBO_BAD_ARGUMENT;
    }
    const size_t nu = u ? (size_t)T * R * de_draws_row(D, NP) : 0;
    for (size_t e = 0; e < nu; ++e)
        if (!(u[e] >= 0.0 && u[e] < 1.0)) {
            set_error("de: draw %zu is %g, outside [0, 1)", e, u[e]);
            return ROBO_BAD_ARGUMENT;
        }
    ROBO_TRY(ensemble_check("de", 0, gps, S, k));
    for (int s = 0; s < S; ++s) {
        if (gps[s]->kind == ROBO_KERNEL_FABOLAS) {
            set_error("de: sample %d has a Fabolas kernel, whose fidelity column is not a box coordinate", s);
            return ROBO_BAD_ARGUMENT;
        }
        for (int t = 0; t < s; ++t)
            if (gps[t] == gps[s]) {
                set_error("de: samples %d and %d share a model handle (one posterior per handle)", t, s);
                return ROBO_BAD_ARGUMENT;
            }
    }
    const int64_t rows = (int64_t)R * NP, m_pad = round_up64(rows, NB);
    if (k->m != rows) {
        set_error("de: %lld candidates for %d instances of %d members (the start is every instance's whole population)",
                  (long long)k->m, R, NP);
        return ROBO_BAD_SHAPE;
    }
    if ((size_t)m_pad * g0->n_pad * sizeof(double) > workspace_bytes(c)) {
        set_error("de: %d rows of %d columns exceed the solve workspace (ws_bytes)", (int)m_pad, g0->n_pad);
        return ROBO_BAD_SHAPE;
    }

    DeState st;
    memset(&st, 0, sizeof(st));
    st.R = R;
    st.D = D;
    st.NP = NP;
    st.T = T;
    st.S = S;
    st.kind = acq_kind;
    st.m_pad = m_pad;
    st.par = par;
    st.f_lo = f_lo;
    st.f_hi = f_hi;
    st.cr = cr;
    st.tol = tol;
    st.atol = atol;
    st.seed = seed;
    st.x0 = k->d_Xc;
    st.f0 = k->d_acq;

    // The solve follows the library's rule for a batch of R NP points (decide_winv): decided, W built and the workspaces
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

    if (!g0->de) {
        g0->de = new DeWork();
        memset(g0->de, 0, sizeof(DeWork));
    }
    DeWork* wk = g0->de;
    // one block: doubles first, then the model records, then the 4-byte words
    const size_t pd = (size_t)rows * D;
    BlockLayout lay(16);
    lay.add(&st.pop, pd);
    lay.add(&st.val, (size_t)rows);
    lay.add(&st.trial, pd);
    lay.add(&st.out, (size_t)D + 3);
    lay.add(&st.u, nu);
    lay.add(&st.model, (size_t)S);
    lay.add(&st.best, (size_t)R);
    lay.add(&st.gen, (size_t)R);
    lay.add(&st.code, (size_t)R);
    lay.add(&st.flags, (size_t)R);
    ROBO_TRY(dev_grow(c->stream, &wk->d_block, &wk->bytes, lay.bytes()));
    lay.bind(wk->d_block);
    if (!u) st.u = nullptr;
    const size_t trace_len = (size_t)(T + 1) * R * de_trace_row(D, NP);
    if (out_trace) ROBO_TRY(dev_grow(c->stream, &wk->d_trace, &wk->trace_cap, trace_len));
    st.trace = out_trace ? wk->d_trace : nullptr;

    // (u and model are const in DeState, the kernels only read them: the uploads cast that away)
    const hipMemcpyKind h2d = hipMemcpyHostToDevice;
    if (nu > 0) ROBO_HIP_CHECK(hipMemcpyAsync((void*)st.u, u, nu * sizeof(double), h2d, c->stream));
    if (T > 0) ROBO_HIP_CHECK(hipMemcpyAsync((void*)st.model, models.data(), (size_t)S * sizeof(CmaModel), h2d, c->stream));

    ROBO_TRY(acq_sweep(gps, S, marginal, acq_kind, par, etas, k));
    // generations, the last select, the winner: launches only
    int status = ROBO_OK;
    for (int g = 0; status == ROBO_OK && g < T; ++g) {
        status = launch_de_step(c, st, g);
        for (int s = 0; status == ROBO_OK && s < S; ++s) status = predict_scaled(gps[s], hs[s], use_w[s] != 0);
    }
    if (status == ROBO_OK) status = launch_de_step(c, st, T);
    if (status == ROBO_OK) status = launch_de_result(c, st, k->d_flags);
    // read-back: the one synchronisation of the call
    std::vector<double> h((size_t)D + 3);
    ROBO_TRY(finish_call(k, "de", status, {{h.data(), st.out, h.size() * sizeof(double)},
                                            {out_generations, st.gen, (size_t)R * sizeof(int32_t)},
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

int32_t robo_acq_de_cand(robo_gp* gp, int32_t acq_kind, double par, double eta, robo_cand* cand, int32_t n_instances,
                         int32_t popsize, int32_t n_generations, double f_lo, double f_hi, double cr, double tol, double atol,
                         const double* u, uint64_t seed, double* out_x, double* out_value, int32_t* out_instance,
                         int32_t* out_generations, uint32_t* out_flags, double* out_trace) {
    return de_core(&gp, gp ? 1 : 0, false, acq_kind, par, &eta, cand, n_instances, popsize, n_generations, f_lo, f_hi, cr, tol,
                   atol, u, seed, out_x, out_value, out_instance, out_generations, out_flags, out_trace);
}

int32_t robo_acq_de_marginal_cand(robo_gp* const* gps, int32_t S, int32_t acq_kind, double par, const double* etas,
                                  robo_cand* cand, int32_t n_instances, int32_t popsize, int32_t n_generations, double f_lo,
                                  double f_hi, double cr, double tol, double atol, const double* u, uint64_t seed,
                                  double* out_x, double* out_value, int32_t* out_instance, int32_t* out_generations,
                                  uint32_t* out_flags, double* out_trace) {
    return de_core(gps, S, true, acq_kind, par, etas, cand, n_instances, popsize, n_generations, f_lo, f_hi, cr, tol, atol, u,
                   seed, out_x, out_value, out_instance, out_generations, out_flags, out_trace);
}

}  // extern "C"
