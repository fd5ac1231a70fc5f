// Entropy search's representer points, sampled on the device (robo_rep_sample, robo_rep_sample_batch).
//
// Replaces the loop InformationGain.sample_representer_points drives from the host (the reference:
// robo/acquisition_functions/information_gain.py:132-151, emcee's EnsembleSampler around one acquisition value per walker):
// 50 ensemble steps x 2 half-steps, each a robo_acq_eval round trip for at most Nb / 2 points -- and under
// MarginalizationGPMCMC the same again for every hyper-parameter sample.  Here S chains (one per fitted model, all on one
// context) advance T steps in lock step with launches only:
//
//   per half-step   rep_propose_kernel   all chains: q = c - z (c - s) for the moving half, the box test, the model's input
//                                        normalisation and the scaling by each model's metrics into its candidate handle
//                   per chain            the posterior of the half's rows -- predict_scaled, i.e. the solve and the post
//                                        kernel robo_acq_eval itself runs for a batch of that size, on the handle behind
//                                        the host-array entry points: the moments have the bits robo_acq_eval returns
//                   rep_accept_kernel    all chains: acquisition value (kern_math.h, as acq_kernel), emcee's accept test,
//                                        walker / log-probability / acceptance-count update, trace
//
// The random numbers do not depend on the chain: the caller draws them up front in emcee 2's order (robo_mcmc_draws).  z, q
// and the normalisation are rn_* operations (common.h), never contracted: they equal NumPy's bit for bit.  A chain never
// looks at another chain, so its result does not depend on S or on its index.
#include <vector>

#include "api_internal.h"
#include "kern_math.h"
#include "mcmc_dev.h"

namespace robo {

// One thread per (row of the handle, coordinate); grid.y = chain.  Rows beyond the half replicate row 0, as
// scale_inputs_kernel's pad rows do.  Every thread of a walker forms the walker's whole proposal for the box test (D is
// small); the thread of coordinate d leaves q_d behind, the one of coordinate 0 also z and the verdict.
// start == 1: the walkers of half h themselves (first evaluation of the start positions)
__global__ __launch_bounds__(256) void rep_propose_kernel(RepState st, int start, int h, int it) {
    const int s = blockIdx.y, D = st.D, half = st.k / 2;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= st.m_pad * D) return;
    const long long r = i / D;
    const int d = (int)(i - r * D);
    const int w = r < half ? (int)r : 0;
    const double* own = st.pos + ((size_t)s * st.k + (size_t)h * half + w) * D;
    double z = 1.0, qd = own[d];
    bool out = false;
    if (start) {
        for (int e = 0; e < D; ++e) out = out || !(own[e] >= st.lower[e] && own[e] <= st.upper[e]);
    } else {
        const size_t draw = (((size_t)s * st.T + it) * 2 + h) * half + w;
        const double* c = st.pos + ((size_t)s * st.k + (size_t)(1 - h) * half + st.partner[draw]) * D;
        z = mcmc_stretch_z(st.a, st.uz[draw]);
        for (int e = 0; e < D; ++e) {
            const double qe = mcmc_stretch_q(c[e], own[e], z);
            out = out || !(qe >= st.lower[e] && qe <= st.upper[e]);        // also true for NaN
            if (e == d) qd = qe;
        }
    }
    if (r < half) {
        st.q[((size_t)s * half + w) * D + d] = qd;
        if (d == 0) {
            st.z[(size_t)s * half + w] = z;
            st.outside[(size_t)s * half + w] = out ? 1 : 0;
        }
    }
    // a walker outside the box hands its own current position to the solve (finite rows); its value is never used
    double x = out ? own[d] : qd;
    if (st.normalize) x = rn_div(rn_sub(x, st.lower[d]), rn_sub(st.upper[d], st.lower[d]));
    const RepChain ch = st.chain[s];
    ch.Xcs[i] = x * ch.ism[d];
}

// One thread per (chain, walker of the moving half)
__global__ __launch_bounds__(64) void rep_accept_kernel(RepState st, int kind, double par, int start, int h, int it) {
    const int s = blockIdx.y, D = st.D, half = st.k / 2;
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= half) return;
    const RepChain ch = st.chain[s];
    const size_t hw = (size_t)s * half + w, sw = (size_t)s * st.k + (size_t)h * half + w;
    const bool out = st.outside[hw] != 0;
    const double ninf = -__builtin_huge_val();
    double lp = ninf;
    if (!out) {
        const double mu = ch.mean[w], v = ch.var[w];
        unsigned f = 0;
        if (kind == ROBO_ACQ_EI) {
            lp = acq_ei(mu, v, ch.eta, par);
            if (lp < 0.0 && lp > -2.2250738585072014e-308) lp = 0.0;    // as acq_kernel
            if (lp < 0.0) f |= ROBO_FLAG_NEGATIVE_EI;
        } else if (kind == ROBO_ACQ_LOG_EI) {
            lp = acq_log_ei(mu, v, ch.eta, par);
        } else if (kind == ROBO_ACQ_PI) {
            lp = acq_pi(mu, v, ch.eta, par);
        } else {
            lp = acq_lcb(mu, v, par);
        }
        if (sqrt(v) == 0.0) f |= ROBO_FLAG_ZERO_SIGMA;
        if (lp != lp) f |= ROBO_FLAG_NAN;                               // emcee: "lnprob returned NaN."
        if (f != 0) atomicOr(st.flags + s, f);
    }
    if (start) {
        st.lnp[sw] = lp;
        return;
    }
    const size_t draw = (((size_t)s * st.T + it) * 2 + h) * half + w;
    const double* q = st.q + hw * D;
    const double lnpdiff = mcmc_lnpdiff(D, log(st.z[hw]), lp, st.lnp[sw]);
    const bool accept = lnpdiff > log(st.ua[draw]);                     // -inf (and NaN) never accepts
    if (accept) {
        for (int d = 0; d < D; ++d) st.pos[sw * D + d] = q[d];
        st.lnp[sw] = lp;
        st.nacc[sw] += 1;
    }
    if (st.trace) {
        double* row = st.trace + draw * (D + 2);
        for (int d = 0; d < D; ++d) row[d] = q[d];
        row[D] = lp;
        row[D + 1] = out ? 2.0 : (accept ? 1.0 : 0.0);
    }
}

int launch_rep_propose(robo_ctx* ctx, const RepState& st, int start, int h, int it) {
    const unsigned blocks = (unsigned)((st.m_pad * st.D + 255) / 256);
    hipLaunchKernelGGL(rep_propose_kernel, dim3(blocks, (unsigned)st.S), dim3(256), 0, ctx->stream, st, start, h, it);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_rep_accept(robo_ctx* ctx, const RepState& st, int acq_kind, double par, int start, int h, int it) {
    const unsigned blocks = (unsigned)((st.k / 2 + 63) / 64);
    hipLaunchKernelGGL(rep_accept_kernel, dim3(blocks, (unsigned)st.S), dim3(64), 0, ctx->stream, st, acq_kind, par, start, h,
                       it);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

void rep_free(RepWork* w) {
    if (!w) return;
    hipFree(w->d_block);
    hipFree(w->d_trace);
    delete w;
}

// ---- the driver ---------------------------------------------------------------------------------------------------------------
static int rep_core(robo_gp* const* gps, int32_t S, int32_t acq_kind, double par, const double* etas, const double* lower,
                    const double* upper, int32_t normalize, int32_t n_walkers, int32_t n_steps, double a,
                    const double* u_stretch, const int32_t* partner, const double* u_accept, double* pos, double* lnp,
                    int32_t eval_start, int64_t* out_accepted, uint32_t* out_flags, double* out_trace) {
    if (!gps || S < 1 || !etas || !lower || !upper || !pos || !lnp) return ROBO_BAD_ARGUMENT;
    if (n_steps > 0 && (!u_stretch || !partner || !u_accept)) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(check_acq_kind(acq_kind));
    for (int s = 0; s < S; ++s)
        if (!gps[s]) return ROBO_BAD_ARGUMENT;
    const int k = n_walkers, T = n_steps, D = gps[0]->dim, half = k / 2;
    if (k < 2 || k % 2 != 0) {
        set_error("rep_sample: the number of walkers must be even (got %d)", k);
        return ROBO_BAD_ARGUMENT;
    }
    if (k < 2 * D) {
        set_error("rep_sample: the number of walkers (%d) needs to be at least twice the dimension (%d)", k, D);
        return ROBO_BAD_ARGUMENT;
    }
    if (T < 0 || !(a > 1.0)) {
        set_error("rep_sample: n_steps %d (>= 0), a %g (> 1)", T, a);
        return ROBO_BAD_ARGUMENT;
    }
    for (int d = 0; d < D; ++d)
        if (!(lower[d] < upper[d])) {
            set_error("rep_sample: lower[%d] = %g is not below upper[%d] = %g", d, lower[d], d, upper[d]);
            return ROBO_BAD_ARGUMENT;
        }
    for (size_t i = 0; i < (size_t)S * T * 2 * half; ++i)
        if (partner[i] < 0 || partner[i] >= half) {
            set_error("rep_sample: partner index %d outside [0, %d)", partner[i], half);
            return ROBO_BAD_ARGUMENT;
        }
    // every chain's half goes through its own model's kept handle, which ensemble_check compares the models against
    robo_gp* g0 = gps[0];
    robo_ctx* c = g0->ctx;
    if (!g0->fitted) {
        set_error("Model has to be trained first!");
        return ROBO_NOT_FITTED;
    }
    const int64_t m_pad = round_up64(half, NB);
    if ((size_t)m_pad * g0->n_pad * sizeof(double) > workspace_bytes(c)) {
        set_error("rep_sample: %d rows of %d columns exceed the solve workspace (ws_bytes)", (int)m_pad, g0->n_pad);
        return ROBO_BAD_SHAPE;
    }
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    robo_cand* k0 = nullptr;
    ROBO_TRY(host_cand_rows(g0, half, &k0));
    ROBO_TRY(ensemble_check("rep_sample", 0, gps, S, k0));
    // The solve follows the library's rule for a batch of k / 2 points (decide_winv): decided, W built and the workspaces
    // sized before the first step -- nothing below waits for the device.
    std::vector<robo_cand*> hs((size_t)S);
    std::vector<char> use_w((size_t)S, 0);
    std::vector<RepChain> chains((size_t)S);
    for (int s = 0; s < S; ++s) {
        for (int t = 0; t < s; ++t)
            if (gps[t] == gps[s]) {
                set_error("rep_sample: chains %d and %d share a model handle (one chain per handle)", t, s);
                return ROBO_BAD_ARGUMENT;
            }
        robo_gp* g = gps[s];
        ROBO_TRY(host_cand_rows(g, half, &hs[s]));
        ROBO_TRY(cand_ensure_workspace(hs[s], g->n_pad, false));
        bool use = false;
        ROBO_TRY(decide_winv(g, hs[s], &use));
        use_w[s] = use ? 1 : 0;
        chains[s] = RepChain{g->d_theta, hs[s]->d_Xcs, hs[s]->d_mean, hs[s]->d_var, etas[s]};
    }

    // one block: doubles first, then the 8-byte integers, then the 4-byte words
    const size_t nd = (size_t)S * T * 2 * half;
    RepState st;
    BlockLayout lay(16);
    lay.add(&st.pos, (size_t)S * k * D);
    lay.add(&st.lnp, (size_t)S * k);
    lay.add(&st.q, (size_t)S * half * D);
    lay.add(&st.z, (size_t)S * half);
    lay.add(&st.uz, nd);
    lay.add(&st.ua, nd);
    lay.add(&st.lower, (size_t)D);
    lay.add(&st.upper, (size_t)D);
    lay.add(&st.nacc, (size_t)S * k);
    lay.add(&st.chain, (size_t)S);
    lay.add(&st.partner, nd);
    lay.add(&st.outside, (size_t)S * half);
    lay.add(&st.flags, (size_t)S);
    if (!g0->rep) g0->rep = new RepWork();
    RepWork* w = g0->rep;
    ROBO_TRY(dev_grow(c->stream, &w->d_block, &w->bytes, lay.bytes()));
    lay.bind(w->d_block);
    const size_t trace_len = nd * ((size_t)D + 2);
    if (out_trace && trace_len > 0) ROBO_TRY(dev_grow(c->stream, &w->d_trace, &w->trace_cap, trace_len));
    st.S = S;
    st.k = k;
    st.D = D;
    st.T = T;
    st.normalize = normalize ? 1 : 0;
    st.m_pad = m_pad;
    st.a = a;
    st.trace = (out_trace && trace_len > 0) ? w->d_trace : nullptr;

    // (uz .. chain are const in RepState, the kernels only read them: the uploads cast that away)
    hipStream_t stream = c->stream;
    const hipMemcpyKind h2d = hipMemcpyHostToDevice;
    ROBO_HIP_CHECK(hipMemcpyAsync(st.pos, pos, (size_t)S * k * D * 8, h2d, stream));
    if (!eval_start) ROBO_HIP_CHECK(hipMemcpyAsync(st.lnp, lnp, (size_t)S * k * 8, h2d, stream));
    if (nd > 0) {
        ROBO_HIP_CHECK(hipMemcpyAsync((void*)st.uz, u_stretch, nd * 8, h2d, stream));
        ROBO_HIP_CHECK(hipMemcpyAsync((void*)st.ua, u_accept, nd * 8, h2d, stream));
        ROBO_HIP_CHECK(hipMemcpyAsync((void*)st.partner, partner, nd * 4, h2d, stream));
    }
    ROBO_HIP_CHECK(hipMemcpyAsync((void*)st.lower, lower, (size_t)D * 8, h2d, stream));
    ROBO_HIP_CHECK(hipMemcpyAsync((void*)st.upper, upper, (size_t)D * 8, h2d, stream));
    ROBO_HIP_CHECK(hipMemcpyAsync((void*)st.chain, chains.data(), (size_t)S * sizeof(RepChain), h2d, stream));
    ROBO_HIP_CHECK(hipMemsetAsync(st.nacc, 0, (size_t)S * k * 8, stream));
    ROBO_HIP_CHECK(hipMemsetAsync(st.flags, 0, (size_t)S * 4, stream));

    // start evaluation and steps: launches only
    int status = ROBO_OK;
    auto half_step = [&](int start, int h, int it) {
        int e = launch_rep_propose(c, st, start, h, it);
        for (int s = 0; e == ROBO_OK && s < S; ++s) e = predict_scaled(gps[s], hs[s], use_w[s] != 0);
        if (e == ROBO_OK) e = launch_rep_accept(c, st, acq_kind, par, start, h, it);
        return e;
    };
    for (int h = 0; eval_start && status == ROBO_OK && h < 2; ++h) status = half_step(1, h, 0);
    for (int it = 0; status == ROBO_OK && it < T; ++it)
        for (int h = 0; status == ROBO_OK && h < 2; ++h) status = half_step(0, h, it);
    // read-back: the one synchronisation of the call
    std::vector<long long> hacc(out_accepted ? (size_t)S * k : 0);
    ROBO_TRY(finish_call(k0, "rep_sample", status, {{pos, st.pos, (size_t)S * k * D * 8},
                                                    {lnp, st.lnp, (size_t)S * k * 8},
                                                    {hacc.empty() ? nullptr : hacc.data(), st.nacc, hacc.size() * 8},
                                                    {out_flags, st.flags, (size_t)S * 4},
                                                    {st.trace ? out_trace : nullptr, w->d_trace, trace_len * 8}}));
    for (size_t i = 0; i < hacc.size(); ++i) out_accepted[i] = (int64_t)hacc[i];
    return ROBO_OK;
}

}  // namespace robo

using namespace robo;

extern "C" {

int32_t robo_rep_sample(robo_gp* gp, int32_t acq_kind, double par, double eta, const double* lower, const double* upper,
                        int32_t normalize, int32_t n_walkers, int32_t n_steps, double a, const double* u_stretch,
                        const int32_t* partner, const double* u_accept, double* pos, double* lnp, int32_t eval_start,
                        int64_t* out_accepted, uint32_t* out_flags, double* out_trace) {
    return rep_core(&gp, gp ? 1 : 0, acq_kind, par, &eta, lower, upper, normalize, n_walkers, n_steps, a, u_stretch, partner,
                    u_accept, pos, lnp, eval_start, out_accepted, out_flags, out_trace);
}

int32_t robo_rep_sample_batch(robo_gp* const* gps, int32_t S, int32_t acq_kind, double par, const double* etas,
                              const double* lower, const double* upper, int32_t normalize, int32_t n_walkers,
                              int32_t n_steps, double a, const double* u_stretch, const int32_t* partner,
                              const double* u_accept, double* pos, double* lnp, int32_t eval_start, int64_t* out_accepted,
                              uint32_t* out_flags, double* out_trace) {
    return rep_core(gps, S, acq_kind, par, etas, lower, upper, normalize, n_walkers, n_steps, a, u_stretch, partner,
                    u_accept, pos, lnp, eval_start, out_accepted, out_flags, out_trace);
}

}  // extern "C"
