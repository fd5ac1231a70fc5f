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

// ---- Phi(z) / h(z), h = z Phi + phi: the factor of dz in d log EI ----------------------------------------------------------
// z >= -1: the plain quotient (h has no cancellation there).  z < -1, t = -z: with the Mills ratio
// M(t) = Phi(-t) / phi(t) = sqrt(pi / 2) erfcx(t / sqrt 2) the quotient is M / (1 - t M), free of underflow; 1 - t M
// ~ 1 / t^2 cancels and amplifies erfcx's rounding by t^2 (relative error ~ t^2 eps: 5.7e-14 at t = 16).  From t = 16 on
// the asymptotic series in u = 1 / t^2
//     t M = 1 - u + 3 u^2 - 15 u^3 + ...,      1 - t M = u (1 - 3 u + 15 u^2 - 105 u^3 + ...)
// is used with 12 terms: the first omitted term is 23!! u^12 = 4e-18 at t = 16 (below one ulp) and falls from there.
constexpr double REFINE_TAIL_T = 16.0;
__device__ __forceinline__ double cdf_over_h(double z) {
    if (z >= -1.0) {
        const double P = norm_cdf(z);
        return P / (z * P + norm_pdf(z));
    }
    const double t = -z;
    if (t < REFINE_TAIL_T) {
        const double M = 1.25331413731550025121 * erfcx(t * SQRT1_2);
        return M / (1.0 - t * M);
    }
    const double u = 1.0 / (t * t);
    double num = 0.0, den = 0.0;       // Horner from the highest term: coefficients (-1)^n (2n - 1)!! and (-1)^n (2n + 1)!!
    double c = 316234143225.0;         // 23!!
    for (int n = 12; n >= 1; --n) {    // c = (2n - 1)!! on entry
        const double sgn = (n & 1) ? -1.0 : 1.0;
        num = (num + sgn * c) * u;
        den = (den + sgn * c * (double)(2 * n + 1)) * u;
        c /= (double)(2 * n - 1);
    }
    // t M = 1 + num,  (1 - t M) / u = 1 + den  ->  M / (1 - t M) = t (1 + num) / (1 + den)
    return t * (1.0 + num) / (1.0 + den);
}

// ---- value + gradient + step: one workgroup per start ----------------------------------------------------------------------
// Rows (k E .. k E + D) of the solved workspace are v = L^-1 k_*(y_k) and w_d = L^-1 dk_*/dxs_d; q / mu are the solve's
// reductions |row|^2 and row . z.  The D dot products v . w_d over the N columns are the memory-bound part: wave w takes
// the rows d = w, w + 4, ..., every lane two adjacent columns per load (16 B), so each w_d row is requested once and v (one
// row, reused D times by the four waves) is expected to come from the cache -- by construction, not measured; with one
// workgroup per start and two FMA chains per lane the kernel is more likely bound by load latency than by bandwidth
// (its measured share of an iteration is in NOTES.md "Gradient refinement on the device").  Then m, v, dm, dv as predgrad_post_kernel forms
// them, the acquisition value and gradient, the sum over hyper-parameter samples (s = 0 .. S - 1 in order, then / S:
// NumPy's axis-0 mean), and after the last sample the accept test and the next trial point.
__global__ __launch_bounds__(256) void refine_eval_kernel(RefineState st, const double* __restrict__ V, int ldv, int ncols,
                                                          const double* __restrict__ q, const double* __restrict__ mu,
                                                          const double* __restrict__ ism, CovParams cp, double mean_c,
                                                          double y_mean, double y_std, int kind, double par, double eta,
                                                          int s, int S, int t, int T) {
    __shared__ double sdot[MAX_DIM];
    __shared__ double sgp[MAX_DIM];
    const int k = blockIdx.x, D = cp.dim, E = D + 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double ninf = -__builtin_huge_val();
    // everything this launch overwrites is read first
    const long long start = st.start[k];
    const int was_frozen = st.frozen[k];
    const double fx = st.f[k], alpha0 = st.alpha[k], aused = st.aused[k];
    const double facc0 = s > 0 ? st.fy[k] : 0.0;
    const int bad0 = s > 0 ? st.bad[k] : 0;
    const bool mine = tid < D;
    const size_t kd = (size_t)k * D + (mine ? tid : 0);
    const double xd0 = st.x[kd], gd0 = st.g[kd], yd = st.y[kd];
    const double gacc0 = s > 0 ? st.gy[kd] : 0.0;

    const double* v0 = V + (size_t)k * E * ldv;
    for (int d = wave; d < D; d += 4) {
        const double* vd = v0 + (size_t)(1 + d) * ldv;
        double a0 = 0.0, a1 = 0.0;
        for (int j = 2 * lane; j < ncols; j += 128) {
            const double2 a = *reinterpret_cast<const double2*>(v0 + j);
            const double2 b = *reinterpret_cast<const double2*>(vd + j);
            a0 = fma(a.x, b.x, a0);
            a1 = fma(a.y, b.y, a1);
        }
        double acc = a0 + a1;
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) sdot[d] = acc;
    }
    __syncthreads();

    // posterior moments at the trial (every thread: a few dozen flops) and this thread's gradient components
    const double u = st.ys[(size_t)k * D + D - 1];
    const double m = (mu[(size_t)k * E] + mean_c) * y_std + y_mean;
    const double vraw = (cov_self(cp, u) - q[(size_t)k * E]) * (y_std * y_std);
    const double eps = 2.220446049250313e-16;
    const bool floored = !(vraw >= eps);
    const double v = floored ? eps : vraw;
    const double sd = sqrt(v);
    double dm = 0.0, dv = 0.0;
    if (mine) {
        const double dself = (cp.kind == ROBO_KERNEL_FABOLAS && tid == D - 1) ? 2.0 * cp.amp * cp.blr_b * u : 0.0;
        dm = mu[(size_t)k * E + 1 + tid] * ism[tid] * y_std;
        dv = (dself - 2.0 * sdot[tid]) * ism[tid] * (y_std * y_std);
    }
    const double ds = dv / (2.0 * sd);
    double f, df;
    if (kind == ROBO_ACQ_LCB) {
        f = acq_lcb(m, v, par);
        df = -(dm - par * ds);
    } else {
        const double z = (eta - m - par) / sd;
        if (kind == ROBO_ACQ_EI) {
            f = acq_ei(m, v, eta, par);
            if (f < 0.0 && f > -2.2250738585072014e-308) f = 0.0;    // as acq_kernel
            df = -dm * norm_cdf(z) + ds * norm_pdf(z);
        } else if (kind == ROBO_ACQ_PI) {
            f = acq_pi(m, v, eta, par);
            df = -(norm_pdf(z) / sd) * (dm + ds * z);
        } else {
            f = acq_log_ei(m, v, eta, par);
            const double dz = (-dm - z * ds) / sd;
            df = ds / sd + cdf_over_h(z) * dz;
        }
    }
    const double facc = s > 0 ? facc0 + f : f;
    const double gacc = s > 0 ? gacc0 + df : df;
    const int bad = bad0 | (floored ? 1 : 0);
    if (s + 1 < S) {               // more samples to come: leave the partial sums behind
        if (mine) st.gy[kd] = gacc;
        if (tid == 0) {
            st.fy[k] = facc;
            st.bad[k] = bad;
        }
        return;
    }
    const double fy = rn_div(facc, (double)S);
    const double gyd = rn_div(gacc, (double)S);

    // the decision (identical in every thread)
    const bool trial_bad = bad != 0 || !isfinite(fy);
    int frozen = was_frozen, code;
    bool accept = false;
    double alpha = alpha0;
    if (start < 0) {
        code = 2;
    } else if (t == 0) {             // the start itself: always the current point
        accept = true;
        code = trial_bad ? 3 : 1;
        if (trial_bad) frozen = 1;
    } else if (was_frozen) {
        code = 2;
    } else if (trial_bad) {          // variance on its floor or value not finite: not taken, and the start stops here
        code = 3;
        frozen = 1;
    } else {
        accept = fy > fx;
        code = accept ? 1 : 0;
        alpha = accept ? fmin(rn_mul(2.0, alpha0), 0.5) : rn_mul(alpha0, 0.5);
    }
    const double xd = accept ? yd : xd0, gd = accept ? gyd : gd0;

    if (st.trace) {
        double* row = st.trace + ((size_t)t * st.K + k) * (2 * D + 3);
        if (mine) {
            row[tid] = yd;
            row[D + 1 + tid] = gyd;
        }
        if (tid == 0) {
            row[D] = fy;
            row[2 * D + 1] = aused;
            row[2 * D + 2] = (double)code;
        }
    }

    // next trial: projected direction of unit length, clipped to the box
    double gp = 0.0;
    if (mine) gp = ((xd <= 0.0 && gd < 0.0) || (xd >= 1.0 && gd > 0.0)) ? 0.0 : gd;
    if (mine) sgp[tid] = gp;
    __syncthreads();
    double n2 = 0.0;
    for (int d = 0; d < D; ++d) n2 += sgp[d] * sgp[d];
    const double nrm = sqrt(n2);
    const bool more = t < T;
    if (more && !frozen && !(nrm > 0.0 && isfinite(nrm))) frozen = 1;    // no ascent direction left inside the box
    if (mine) {
        double yn = xd;
        if (more && !frozen) {
            yn = rn_add(xd, rn_div(rn_mul(alpha, gp), nrm));
            yn = yn < 0.0 ? 0.0 : (yn > 1.0 ? 1.0 : yn);
        }
        st.y[kd] = yn;
        if (accept) {
            st.x[kd] = xd;
            st.g[kd] = gd;
        }
    }
    if (tid == 0) {
        if (accept) st.f[k] = fy;
        else if (start < 0) st.f[k] = ninf;
        st.alpha[k] = alpha;
        st.aused[k] = alpha;
        st.frozen[k] = frozen;
        if (frozen && !was_frozen) atomicOr(st.flags, ROBO_FLAG_FROZEN);
    }
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

int launch_refine_result(robo_ctx* ctx, const RefineState& st, unsigned* d_cand_flags, bool sweep_only) {
    hipLaunchKernelGGL(refine_result_kernel, dim3(1), dim3(64), 0, ctx->stream, st, d_cand_flags, sweep_only ? 1 : 0);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

// ---- the driver ---------------------------------------------------------------------------------------------------------------
// state + pseudo-row workspace for K starts in D dimensions, kept with the GP like the host-array candidate handle
static int refine_ensure(robo_gp* g, int K, int D, RefineWork** out) {
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

// marginal: the sweep is robo_acq_eval_marginal_cand's (accumulate, divide); otherwise robo_acq_eval_cand's
static int refine_core(robo_gp* const* gps, int32_t S, bool marginal, int32_t acq_kind, double par, const double* etas,
                       robo_cand* k, int32_t n_starts, int32_t n_steps, double step0, double* out_x, double* out_value,
                       int64_t* out_start_index, uint32_t* out_flags, int64_t* out_starts, double* out_trace) {
    if (!gps || S < 1 || !etas || !k || !out_x) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(check_acq_kind(acq_kind));
    if (n_starts < 1 || n_starts > 1024 || n_steps < 0 || !(step0 > 0.0) || !(step0 <= 0.5)) {
        set_error("refine: n_starts %d (1 .. 1024), n_steps %d (>= 0), step0 %g (0 < step0 <= 0.5)", n_starts, n_steps, step0);
        return ROBO_BAD_ARGUMENT;
    }
    ROBO_TRY(ensemble_check("refine", 0, gps, S, k));
    robo_gp* g0 = gps[0];
    robo_ctx* c = g0->ctx;
    const int K = n_starts, T = n_steps, D = g0->dim, E = D + 1;
    const int64_t rows_pad = round_up64((int64_t)K * E, NB);
    if ((size_t)rows_pad * g0->n_pad * sizeof(double) > workspace_bytes(c)) {
        set_error("refine: %d starts x %d rows of %d columns exceed the solve workspace (ws_bytes)", K, E, g0->n_pad);
        return ROBO_BAD_SHAPE;
    }
    RefineWork* w = nullptr;
    ROBO_TRY(refine_ensure(g0, K, D, &w));
    ROBO_TRY(cand_ensure_workspace(w->ws, g0->n_pad, true));
    const size_t trace_len = (size_t)(T + 1) * K * (2 * D + 3);
    if (out_trace) ROBO_TRY(dev_grow(c->stream, &w->d_trace, &w->trace_cap, trace_len));
    w->st.trace = out_trace ? w->d_trace : nullptr;
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
            status = launch_scale_inputs(c, st.y, st.ys, g->d_theta, K, K, D);
            if (status == ROBO_OK) status = launch_cross_grad(g, st.ys, use_w[s] ? d_rhs : w->ws->d_V, 0, K, rows_pad);
            if (status == ROBO_OK) status = use_w[s] ? launch_winv_rows(g, w->ws, rows_pad) : launch_trsm(g, w->ws, 0, rows_pad);
            if (status == ROBO_OK) status = launch_refine_eval(g, st, w->ws, acq_kind, par, etas[s], s, S, t, T);
        }
    }
    if (status == ROBO_OK) status = launch_refine_result(c, st, k->d_flags, T == 0);
    // read-back: the one synchronisation of the call
    std::vector<double> h((size_t)D + 4);
    std::vector<long long> hs(out_starts ? (size_t)K : 0);
    ROBO_TRY(finish_call(k, "refine", status, {{h.data(), st.out, h.size() * sizeof(double)},
                                               {hs.data(), st.start, hs.size() * sizeof(long long)},
                                               {out_trace, w->d_trace, trace_len * sizeof(double)}}));
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
