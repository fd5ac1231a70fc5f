// Multi-start gradient refinement of an acquisition maximum, resident on the device (robo_acq_refine_cand,
// robo_acq_refine_marginal_cand; the reference has no such maximiser: its RandomSampling returns a candidate, its
// SciPyOptimizer runs L-BFGS-B with finite differences from the host, one 1 x D call per function value).
//
//   sweep (acq.hip, unchanged)  ->  select_*: the K best candidates, deterministic  ->  refine_gather_kernel
//   ->  (T + 1) x [ scale_inputs, cross_grad_kernel (predgrad.hip), the solve (W = L^-1 product, winv.hip, or block rows, predict.hip),
//                   refine_eval_kernel: value + gradient + accept test + next trial ]  ->  refine_result_kernel
//
// Nothing between the sweep and the read-back touches the host: the state of every start lives in RefineState.
// Every start is one workgroup of the epilogue and never looks at another start, so its trajectory does not depend on K
// or on its slot.  The decisions a host restatement must reproduce (accept test, step-length update, the trial point
// and its clip) are single rn_* operations on stored doubles (common.h), never contracted.
#include <vector>

#include "api_internal.h"
#include "kern_math.h"
#include "refine_eval.h"

namespace robo {

// ---- selection of the K largest values ---------------------------------------------------------------------------------
// Order: descending value, ties by ascending index, NaN never.  Every eligible candidate gets the 96-bit key
// (hi = order-preserving bits of the value with -0 read as +0, lo = ~index): keys are pairwise distinct and "better" is
// "larger".  The K-th largest key is found by a most-significant-digit radix selection, 8 bits per pass (8 passes over
// the value, 4 over the index): a histogram of the digit among the keys that share the digits fixed so far (integer
// counts: the same whatever order the workgroups run in), then one thread walks the 256 counts from the top.  The K keys
// >= the threshold are collected in arrival order and sorted by rank counting, which is a permutation because the keys
// are distinct: the result is a function of the values alone.
constexpr int SEL_PASSES = 12;

__device__ __forceinline__ unsigned long long sel_key_hi(double v) {
    const long long b = __double_as_longlong(v == 0.0 ? 0.0 : v);
    const unsigned long long u = (unsigned long long)b;
    return b < 0 ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ unsigned sel_key_lo(long long i) { return ~(unsigned)i; }

__device__ __forceinline__ unsigned sel_digit(unsigned long long hi, unsigned lo, int pass) {
    return pass < 8 ? (unsigned)(hi >> (56 - 8 * pass)) & 255u : (lo >> (24 - 8 * (pass - 8))) & 255u;
}
// do the digits above `pass` equal the threshold's?
__device__ __forceinline__ bool sel_prefix_match(unsigned long long hi, unsigned lo, const RefineSel& s, int pass) {
    if (pass == 0) return true;
    if (pass < 8) return (hi >> (64 - 8 * pass)) == (s.hi >> (64 - 8 * pass));
    if (hi != s.hi) return false;
    if (pass == 8) return true;
    return (lo >> (32 - 8 * (pass - 8))) == (s.lo >> (32 - 8 * (pass - 8)));
}

__global__ __launch_bounds__(256) void select_hist_kernel(const double* __restrict__ vals, long long m, int pass,
                                                          const RefineSel* __restrict__ sel, unsigned* __restrict__ hist) {
    __shared__ unsigned sh[256];
    sh[threadIdx.x] = 0u;
    __syncthreads();
    const RefineSel s = *sel;
    if (pass == 0 || s.remaining > 0u) {
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < m; i += (long long)gridDim.x * 256) {
            const double v = vals[i];
            if (v != v) continue;
            const unsigned long long hi = sel_key_hi(v);
            const unsigned lo = sel_key_lo(i);
            if (sel_prefix_match(hi, lo, s, pass)) atomicAdd(&sh[sel_digit(hi, lo, pass)], 1u);
        }
    }
    __syncthreads();
    if (sh[threadIdx.x] != 0u) atomicAdd(&hist[threadIdx.x], sh[threadIdx.x]);
}

// one thread: fix the digit of this pass, clear the histogram for the next one
__global__ void select_pick_kernel(RefineSel* __restrict__ sel, unsigned* __restrict__ hist, int pass, unsigned K) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    RefineSel s = *sel;
    if (pass == 0) {
        unsigned long long total = 0;
        for (int d = 0; d < 256; ++d) total += hist[d];
        s.keff = total < K ? (unsigned)total : K;
        s.remaining = s.keff;
        s.hi = 0ull;
        s.lo = 0u;
        s.count = 0u;
    }
    if (s.remaining > 0u) {
        unsigned above = 0u;
        int digit = 0;
        for (int d = 255; d >= 0; --d) {
            const unsigned c = hist[d];
            if (above + c >= s.remaining) {
                digit = d;
                break;
            }
            above += c;
        }
        s.remaining -= above;
        if (pass < 8) s.hi |= (unsigned long long)digit << (56 - 8 * pass);
        else s.lo |= (unsigned)digit << (24 - 8 * (pass - 8));
    }
    for (int d = 0; d < 256; ++d) hist[d] = 0u;
    *sel = s;
}

__global__ __launch_bounds__(256) void select_collect_kernel(const double* __restrict__ vals, long long m,
                                                             RefineSel* __restrict__ sel, double* __restrict__ out_val,
                                                             long long* __restrict__ out_idx, unsigned K) {
    const unsigned long long thi = sel->hi;
    const unsigned tlo = sel->lo, keff = sel->keff;
    if (keff == 0u) return;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < m; i += (long long)gridDim.x * 256) {
        const double v = vals[i];
        if (v != v) continue;
        const unsigned long long hi = sel_key_hi(v);
        const unsigned lo = sel_key_lo(i);
        if (hi > thi || (hi == thi && lo >= tlo)) {
            const unsigned slot = atomicAdd(&sel->count, 1u);
            if (slot < K) {
                out_val[slot] = v;
                out_idx[slot] = i;
            }
        }
    }
}

// one workgroup: rank of every collected key among the collected keys -> its place in the sorted list
__global__ __launch_bounds__(256) void select_sort_kernel(const RefineSel* __restrict__ sel,
                                                          const double* __restrict__ in_val,
                                                          const long long* __restrict__ in_idx,
                                                          double* __restrict__ out_val, long long* __restrict__ out_idx) {
    const int keff = (int)sel->keff;
    for (int i = threadIdx.x; i < keff; i += 256) {
        const unsigned long long hi = sel_key_hi(in_val[i]);
        const unsigned lo = sel_key_lo(in_idx[i]);
        int rank = 0;
        for (int j = 0; j < keff; ++j) {
            const unsigned long long hj = sel_key_hi(in_val[j]);
            const unsigned lj = sel_key_lo(in_idx[j]);
            rank += (hj > hi || (hj == hi && lj > lo)) ? 1 : 0;
        }
        out_val[rank] = in_val[i];
        out_idx[rank] = in_idx[i];
    }
}

// start k := the k-th selected candidate (one workgroup per start); slots beyond the eligible candidates stay unused
__global__ __launch_bounds__(64) void refine_gather_kernel(RefineState st, const double* __restrict__ Xc, double step0) {
    const int k = blockIdx.x, D = st.D;
    const bool used = k < (int)st.sel->keff;
    const long long idx = used ? st.sel_idx[st.K + k] : -1;
    for (int d = threadIdx.x; d < D; d += 64) {
        const double v = used ? Xc[(size_t)idx * D + d] : 0.0;
        st.x[(size_t)k * D + d] = v;
        st.y[(size_t)k * D + d] = v;
        st.g[(size_t)k * D + d] = 0.0;
    }
    if (threadIdx.x == 0) {
        st.start[k] = idx;
        st.f[k] = used ? st.sel_val[st.K + k] : -__builtin_huge_val();   // the sweep's value until the first evaluation
        st.alpha[k] = step0;
        st.aused[k] = step0;
        st.frozen[k] = used ? 0 : 1;
        st.bad[k] = 0;
    }
}

// ---- value + gradient + step: one workgroup per start ----------------------------------------------------------------------
// The parts are refine_eval.h's: what the launch overwrites is read first, the D dot products and m, v, dm, dv, then the
// acquisition value and gradient; here the sum over hyper-parameter samples (s = 0 .. S - 1 in order, then / S: NumPy's
// axis-0 mean), and after the last sample the accept test and the next trial point.
__global__ __launch_bounds__(256) void refine_eval_kernel(RefineState st, const double* __restrict__ V, int ldv, int ncols,
                                                          const double* __restrict__ q, const double* __restrict__ mu,
                                                          const double* __restrict__ ism, CovParams cp, double mean_c,
                                                          double y_mean, double y_std, int kind, double par, double eta,
                                                          int s, int S, int t, int T) {
    __shared__ double sdot[MAX_DIM];
    __shared__ double sgp[MAX_DIM];
    const int k = blockIdx.x, D = cp.dim, tid = threadIdx.x;
    const RefineCarried c = refine_carried(st, k, D, tid, s > 0);
    const RefineMoments p = refine_moments(st, k, tid, c.mine, V, ldv, ncols, q, mu, ism, cp, mean_c, y_mean, y_std, sdot);
    double f, df;
    refine_acq(kind, par, eta, p, &f, &df);
    const double facc = s > 0 ? c.facc0 + f : f;
    const double gacc = s > 0 ? c.gacc0 + df : df;
    const int bad = c.bad0 | (p.floored ? 1 : 0);
    if (s + 1 < S) {               // more samples to come: leave the partial sums behind
        if (c.mine) st.gy[c.kd] = gacc;
        if (tid == 0) {
            st.fy[k] = facc;
            st.bad[k] = bad;
        }
        return;
    }
    refine_step(st, k, tid, D, c, rn_div(facc, (double)S), rn_div(gacc, (double)S), bad, t, T, sgp);
}

// the start with the largest final value, first index on ties (NaN only if nothing else is there) -> st.out; the flag
// words of the candidate handle (the sweep's) and of the refinement are reported and cleared
__global__ void refine_result_kernel(RefineState st, unsigned* __restrict__ cand_flags, int sweep_only) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int D = st.D, keff = (int)st.sel->keff;
    unsigned flags = *cand_flags | *st.flags;
    *cand_flags = 0u;
    *st.flags = 0u;
    int best = keff > 0 ? 0 : -1;
    if (!sweep_only) {
        for (int k = 1; k < keff; ++k) {
            const double a = st.f[k], b = st.f[best];
            if ((b != b && a == a) || a > b) best = k;
        }
    }
    const double nan = __longlong_as_double(0x7FF8000000000000LL);
    for (int d = 0; d < D; ++d) st.out[d] = best >= 0 ? st.x[(size_t)best * D + d] : 0.0;
    // without steps the answer is the sweep's own: its argmax and the value the sweep computed for it
    const double value = best >= 0 ? (sweep_only ? st.sel_val[st.K] : st.f[best]) : nan;
    if (value != value) flags |= ROBO_FLAG_NAN;
    st.out[D] = value;
    st.out[D + 1] = __longlong_as_double(best >= 0 ? st.start[best] : -1LL);
    st.out[D + 2] = __longlong_as_double((long long)flags);
    st.out[D + 3] = __longlong_as_double((long long)keff);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
int refine_alloc(robo_ctx* ctx, int K, int D, RefineWork** out) {
    RefineWork* w = new RefineWork();
    w->K = K;
    w->D = D;
    RefineState& st = w->st;
    const size_t kd = (size_t)K * D, k8 = (size_t)round_up(K, 8);
    // doubles first, then the 8-byte integers, then the 4-byte words
    BlockLayout lay(16);
    lay.add(&st.x, kd);
    lay.add(&st.g, kd);
    lay.add(&st.y, kd);
    lay.add(&st.ys, kd);
    lay.add(&st.gy, kd);
    lay.add(&st.f, k8);
    lay.add(&st.alpha, k8);
    lay.add(&st.aused, k8);
    lay.add(&st.fy, k8);
    lay.add(&st.sel_val, 2 * k8);         // sel_val / sel_idx: [0, K) as collected, [K, 2 K) sorted
    lay.add(&st.out, (size_t)D + 4);
    lay.add(&st.start, k8);
    lay.add(&st.sel_idx, 2 * k8);
    lay.add(&st.frozen, k8);
    lay.add(&st.bad, k8);
    lay.add(&st.hist, 256);
    lay.add(&st.flags, 4);
    lay.add(&st.sel, 1);
    const size_t bytes = lay.bytes();
    if (hipMalloc((void**)&w->d_block, bytes) != hipSuccess) {
        set_error("hipMalloc of %zu bytes failed (refinement state)", bytes);
        delete w;
        return ROBO_RUNTIME_ERROR;
    }
    if (hipMemsetAsync(w->d_block, 0, bytes, ctx->stream) != hipSuccess) {
        set_error("hipMemsetAsync of the refinement state failed");
        hipFree(w->d_block);
        delete w;
        return ROBO_RUNTIME_ERROR;
    }
    lay.bind(w->d_block);
    st.K = K;
    st.D = D;
    *out = w;
    return ROBO_OK;
}

void refine_free(RefineWork* w) {
    if (!w) return;
    hipFree(w->d_block);
    hipFree(w->d_trace);
    delete w;
}

int launch_refine_select(robo_ctx* ctx, const RefineState& st, const double* d_vals, int64_t m, const double* d_Xc,
                         double step0) {
    int blocks = (int)((m + 255) / 256);
    if (blocks > 1024) blocks = 1024;
    hipStream_t s = ctx->stream;
    ROBO_HIP_CHECK(hipMemsetAsync(st.hist, 0, 256 * sizeof(unsigned), s));   // (every pick kernel leaves it cleared, too)
    for (int pass = 0; pass < SEL_PASSES; ++pass) {
        hipLaunchKernelGGL(select_hist_kernel, dim3(blocks), dim3(256), 0, s, d_vals, (long long)m, pass,
                           (const RefineSel*)st.sel, st.hist);
        hipLaunchKernelGGL(select_pick_kernel, dim3(1), dim3(64), 0, s, st.sel, st.hist, pass, (unsigned)st.K);
    }
    hipLaunchKernelGGL(select_collect_kernel, dim3(blocks), dim3(256), 0, s, d_vals, (long long)m, st.sel, st.sel_val,
                       st.sel_idx, (unsigned)st.K);
    hipLaunchKernelGGL(select_sort_kernel, dim3(1), dim3(256), 0, s, (const RefineSel*)st.sel, (const double*)st.sel_val,
                       (const long long*)st.sel_idx, st.sel_val + st.K, st.sel_idx + st.K);
    hipLaunchKernelGGL(refine_gather_kernel, dim3((unsigned)st.K), dim3(64), 0, s, st, d_Xc, step0);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_refine_eval(robo_gp* gp, const RefineState& st, const robo_cand* ws, int acq_kind, double par, double eta, int s,
                       int S, int t, int T) {
    const int ncols = (gp->n + NB - 1) / NB * NB;        // the block rows the solve touched
    hipLaunchKernelGGL(refine_eval_kernel, dim3((unsigned)st.K), dim3(256), 0, gp->ctx->stream, st, (const double*)ws->d_V,
                       gp->n_pad, ncols, (const double*)ws->d_q, (const double*)ws->d_mu, (const double*)gp->d_theta,
                       gp->cov, gp->mean_c, gp->y_mean, gp->y_std, acq_kind, par, eta, s, S, t, T);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

// the pending trial points of all K starts against g: scaled with its metrics, value and gradient rows of the cross-covariance,
// the solve -- through W = L^-1 when d_rhs (winv_rows_buffer's) is given, else by block rows -- into w->ws
int launch_refine_solve(robo_gp* g, RefineWork* w, int K, double* d_rhs) {
    const RefineState& st = w->st;
    const int64_t rows_pad = round_up64((int64_t)K * (st.D + 1), NB);
    ROBO_TRY(launch_scale_inputs(g->ctx, st.y, st.ys, g->d_theta, K, K, st.D));
    ROBO_TRY(launch_cross_grad(g, st.ys, d_rhs ? d_rhs : w->ws->d_V, 0, K, rows_pad));
    return d_rhs ? launch_winv_rows(g, w->ws, rows_pad) : launch_trsm(g, w->ws, 0, rows_pad);
}

int launch_refine_result(robo_ctx* ctx, const RefineState& st, unsigned* d_cand_flags, bool sweep_only) {
    hipLaunchKernelGGL(refine_result_kernel, dim3(1), dim3(64), 0, ctx->stream, st, d_cand_flags, sweep_only ? 1 : 0);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

// ---- the driver ---------------------------------------------------------------------------------------------------------------
// state + pseudo-row workspace for K starts in D dimensions, kept with the GP like the host-array candidate handle
int refine_ensure(robo_gp* g, int K, int D, RefineWork** out) {
    if (g->refine && (g->refine->K != K || g->refine->D != D)) {
        ROBO_HIP_CHECK(hipStreamSynchronize(g->ctx->stream));
        robo_cand_destroy(g->refine->ws);
        refine_free(g->refine);
        g->refine = nullptr;
    }
    if (!g->refine) {
        RefineWork* w = nullptr;
        ROBO_TRY(refine_alloc(g->ctx, K, D, &w));
        const int st = cand_alloc(g->ctx, round_up64((int64_t)K * (D + 1), NB), 1, &w->ws);
        if (st != ROBO_OK) {
            refine_free(w);
            return st;
        }
        g->refine = w;
    }
    *out = g->refine;
    return ROBO_OK;
}

int refine_check_steps(int32_t n_starts, int32_t n_steps, double step0) {
    if (n_starts < 1 || n_starts > 1024 || n_steps < 0 || !(step0 > 0.0) || !(step0 <= 0.5)) {
        set_error("refine: n_starts %d (1 .. 1024), n_steps %d (>= 0), step0 %g (0 < step0 <= 0.5)", n_starts, n_steps, step0);
        return ROBO_BAD_ARGUMENT;
    }
    return ROBO_OK;
}

int refine_prepare(robo_gp* holder, int n_pad, int K, int T, bool want_trace, RefineWork** out) {
    robo_ctx* c = holder->ctx;
    const int D = holder->dim, E = D + 1;
    const int64_t rows_pad = round_up64((int64_t)K * E, NB);
    if ((size_t)rows_pad * n_pad * sizeof(double) > workspace_bytes(c)) {
        set_error("refine: %d starts x %d rows of %d columns exceed the solve workspace (ws_bytes)", K, E, n_pad);
        return ROBO_BAD_SHAPE;
    }
    RefineWork* w = nullptr;
    ROBO_TRY(refine_ensure(holder, K, D, &w));
    ROBO_TRY(cand_ensure_workspace(w->ws, n_pad, true));
    if (want_trace) ROBO_TRY(dev_grow(c->stream, &w->d_trace, &w->trace_cap, refine_trace_len(K, T, D)));
    w->st.trace = want_trace ? w->d_trace : nullptr;
    *out = w;
    return ROBO_OK;
}

int refine_read_back(robo_cand* k, RefineWork* w, int status, int T, double* out_x, double* out_value,
                     int64_t* out_start_index, uint32_t* out_flags, int64_t* out_starts, double* out_trace) {
    const RefineState& st = w->st;
    const int K = st.K, D = st.D;
    if (status == ROBO_OK) status = launch_refine_result(k->ctx, st, k->d_flags, T == 0);
    // read-back: the one synchronisation of the call
    std::vector<double> h((size_t)D + 4);
    std::vector<long long> hs(out_starts ? (size_t)K : 0);
    ROBO_TRY(finish_call(k, "refine", status, {{h.data(), st.out, h.size() * sizeof(double)},
                                               {hs.data(), st.start, hs.size() * sizeof(long long)},
                                               {out_trace, w->d_trace, refine_trace_len(K, T, D) * sizeof(double)}}));
    memcpy(out_x, h.data(), (size_t)D * sizeof(double));
    if (out_value) *out_value = h[D];
    long long v;
    memcpy(&v, &h[D + 1], sizeof(v));
    if (out_start_index) *out_start_index = (int64_t)v;
    memcpy(&v, &h[D + 2], sizeof(v));
    if (out_flags) *out_flags = (uint32_t)v;
    for (size_t i = 0; i < hs.size(); ++i) out_starts[i] = (int64_t)hs[i];
    return ROBO_OK;
}

// marginal: the sweep is robo_acq_eval_marginal_cand's (accumulate, divide); otherwise robo_acq_eval_cand's
static int refine_core(robo_gp* const* gps, int32_t S, bool marginal, int32_t acq_kind, double par, const double* etas,
                       robo_cand* k, int32_t n_starts, int32_t n_steps, double step0, double* out_x, double* out_value,
                       int64_t* out_start_index, uint32_t* out_flags, int64_t* out_starts, double* out_trace) {
    if (!gps || S < 1 || !etas || !k || !out_x) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(check_acq_kind(acq_kind));
    ROBO_TRY(refine_check_steps(n_starts, n_steps, step0));
    ROBO_TRY(ensemble_check("refine", 0, gps, S, k));
    robo_gp* g0 = gps[0];
    robo_ctx* c = g0->ctx;
    const int K = n_starts, T = n_steps, D = g0->dim;
    const int64_t rows_pad = round_up64((int64_t)K * (D + 1), NB);
    RefineWork* w = nullptr;
    ROBO_TRY(refine_prepare(g0, g0->n_pad, K, T, out_trace != nullptr, &w));
    const RefineState& st = w->st;

    ROBO_TRY(acq_sweep(gps, S, marginal, acq_kind, par, etas, k));
    // The solve of the K (D + 1) rows follows the library's rule for a batch of that many rows (decide_winv): through the
    // explicit inverse factor where the factor qualifies (one triangular product per pass), else the block-row substitution
    // (n / 128 dependent launches).  Decided, and W built, before the first iteration: nothing below waits for the device.
    const bool iterate = T > 0 || out_trace;
    std::vector<char> use_w((size_t)S, 0);
    double* d_rhs = nullptr;
    for (int s = 0; iterate && s < S; ++s) {
        bool use = false;
        ROBO_TRY(clear_flags_on_error(k, decide_winv(gps[s], w->ws, &use)));
        use_w[s] = use ? 1 : 0;
        if (use && !d_rhs) ROBO_TRY(clear_flags_on_error(k, winv_rows_buffer(gps[s], w->ws, rows_pad, &d_rhs)));
    }
    // starts, iterations, winner: launches only
    int status = launch_refine_select(c, st, k->d_acq, k->m, k->d_Xc, step0);
    for (int t = 0; status == ROBO_OK && iterate && t <= T; ++t) {
        for (int s = 0; status == ROBO_OK && s < S; ++s) {
            robo_gp* g = gps[s];
            status = launch_refine_solve(g, w, K, use_w[s] ? d_rhs : nullptr);
            if (status == ROBO_OK) status = launch_refine_eval(g, st, w->ws, acq_kind, par, etas[s], s, S, t, T);
        }
    }
    return refine_read_back(k, w, status, T, out_x, out_value, out_start_index, out_flags, out_starts, out_trace);
}

}  // namespace robo

using namespace robo;

extern "C" {

int32_t robo_acq_refine_cand(robo_gp* g, int32_t acq_kind, double par, double eta, robo_cand* k, int32_t n_starts,
                             int32_t n_steps, double step0, double* out_x, double* out_value, int64_t* out_start_index,
                             uint32_t* out_flags, int64_t* out_starts, double* out_trace) {
    return refine_core(&g, g ? 1 : 0, false, acq_kind, par, &eta, k, n_starts, n_steps, step0, out_x, out_value,
                       out_start_index, out_flags, out_starts, out_trace);
}

int32_t robo_acq_refine_marginal_cand(robo_gp* const* gps, int32_t S, int32_t acq_kind, double par, const double* etas,
                                      robo_cand* k, int32_t n_starts, int32_t n_steps, double step0, double* out_x,
                                      double* out_value, int64_t* out_start_index, uint32_t* out_flags,
                                      int64_t* out_starts, double* out_trace) {
    return refine_core(gps, S, true, acq_kind, par, etas, k, n_starts, n_steps, step0, out_x, out_value, out_start_index,
                       out_flags, out_starts, out_trace);
}

}  // extern "C"
