// Differential evolution over a closed-form acquisition, resident on the device: the kernels (robo_acq_de_cand,
// robo_acq_de_marginal_cand; the rule is stated in include/robo_hip.h, the driver is api_de.hip).
//
// The reference's DifferentialEvolution maximiser (robo/maximizers/differential_evolution.py) drives SciPy from the host, one
// 1 x D acquisition call per function value.  Here R independent best1bin populations of NP members advance in lock step, one
// workgroup of 256 lanes per instance, and a generation is ONE launch of ours around the posterior of its R NP trial rows:
//
//   de_step_kernel(g)   the instance's population (NP x D) and values into LDS with coalesced reads, then
//                       (a) select: generation g - 1's trial values from the models' resident moments (mean over the models in
//                           order), lane per member; an accepted member's row is taken from the pending trials, lane per
//                           coordinate, in LDS and -- accepted rows only -- in memory
//                       (b) the best member and SciPy's convergence test: two-stage sums of a fixed shape in LDS
//                       (c) generation g's trials: the draws with a lane per member, then a lane per (member, coordinate) in row
//                           order forms t = best + F (x_a - x_b) with all three gathers from LDS, crosses, repairs and stores
//                           the row, scaled by every model's metrics, into that model's candidate handle (coalesced)
//                       g = 0 skips (a) and reads the start from the candidate handle and the sweep's values; g = T skips (c):
//                       it is the last select
//   (per model)         the posterior of the R NP rows: predict_scaled, as robo_acq_eval runs it for such a batch
//   de_result_kernel    the best member of the best instance, the flag words
//
// LDS: the population (128 KB at NP D = 16384) + values, the draws' indices, the reduction scratch: 153 KB of the 160 KB of
// a gfx950 CU, one workgroup per CU, R <= 64 of 256 CUs busy.  There is no product in this algorithm -- a trial is a gather and
// three flops per coordinate -- so nothing here is on the matrix pipe; the posterior's own kernels are.  No atomics: every word
// of the state has one writer, the instance's workgroup.  An instance never looks at another one.
#include "kern_math.h"
#include "philox.h"

namespace robo {

constexpr double DE_DBL_MAX = 1.79769313486231570e308;
constexpr unsigned DE_W_FLAGS = 0xFFFFu, DE_W_TRIAL = 0x10000u, DE_W_NOT_FINITE = 0x20000u;    // bits of the reduced word
constexpr int DE_IDX_NONE = 0x7FFFFFFF;

// the acquisition value of row `at` of the models' handles: summed over the models in order and divided by S, guards as
// acq_kernel's (acq.hip acq_value)
__device__ __forceinline__ double de_value(const DeState& st, size_t at, unsigned& f) {
    double facc = 0.0;
    for (int s = 0; s < st.S; ++s) {
        const CmaModel md = st.model[s];
        const double mean = md.mean[at], v = md.var[at];
        double a;
        if (st.kind == ROBO_ACQ_EI) {
            a = acq_ei(mean, v, md.eta, st.par);
            if (a < 0.0 && a > -2.2250738585072014e-308) a = 0.0;
            if (a < 0.0) f |= ROBO_FLAG_NEGATIVE_EI;
        } else if (st.kind == ROBO_ACQ_LOG_EI) {
            a = acq_log_ei(mean, v, md.eta, st.par);
        } else if (st.kind == ROBO_ACQ_PI) {
            a = acq_pi(mean, v, md.eta, st.par);
        } else {
            a = acq_lcb(mean, v, st.par);
        }
        if (sqrt(v) == 0.0) f |= ROBO_FLAG_ZERO_SIGMA;
        if (a != a) f |= ROBO_FLAG_NAN;
        facc = s > 0 ? rn_add(facc, a) : a;
    }
    const double val = rn_div(facc, (double)st.S);
    if (val != val) f |= ROBO_FLAG_NAN;
    return val;
}

// The rule's two-stage sum: partial j takes term(i) of the members i = j, j + 256, ... in increasing i, the partials are added
// by the tree j += j + stride, stride = 128 .. 1 -> every lane.  sRed: WG entries.
template <class Term>
__device__ __forceinline__ double de_sum(double* sRed, int NP, Term term) {
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < NP; i += WG) acc = rn_add(acc, term(i));
    sRed[tid] = acc;
    __syncthreads();
    for (int o = WG / 2; o > 0; o >>= 1) {
        if (tid < o) sRed[tid] = rn_add(sRed[tid], sRed[tid + o]);
        __syncthreads();
    }
    const double s = sRed[0];
    __syncthreads();
    return s;
}

// the OR of every lane's word -> every lane; sRedI: WG entries
__device__ __forceinline__ unsigned de_or(int* sRedI, unsigned w) {
    const int tid = threadIdx.x;
    sRedI[tid] = (int)w;
    __syncthreads();
    for (int o = WG / 2; o > 0; o >>= 1) {
        if (tid < o) sRedI[tid] |= sRedI[tid + o];
        __syncthreads();
    }
    const unsigned all = (unsigned)sRedI[0];
    __syncthreads();
    return all;
}

// the member with the largest value, ties to the lowest index, NaN never; every value NaN: member 0 -> every lane
__device__ __forceinline__ int de_best(const double* sVal, double* sRed, int* sRedI, int NP) {
    const int tid = threadIdx.x;
    double bv = 0.0;
    int bi = DE_IDX_NONE;
    for (int i = tid; i < NP; i += WG) {
        const double v = sVal[i];
        if (v == v && (bi == DE_IDX_NONE || v > bv)) {
            bv = v;
            bi = i;
        }
    }
    sRed[tid] = bv;
    sRedI[tid] = bi;
    __syncthreads();
    for (int o = WG / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const double v = sRed[tid + o];
            const int i = sRedI[tid + o];
            if (i != DE_IDX_NONE && (sRedI[tid] == DE_IDX_NONE || v > sRed[tid] || (v == sRed[tid] && i < sRedI[tid]))) {
                sRed[tid] = v;
                sRedI[tid] = i;
            }
        }
        __syncthreads();
    }
    const int best = sRedI[0] == DE_IDX_NONE ? 0 : sRedI[0];
    __syncthreads();
    return best;
}

// floor(u n) for u in [0, 1), never above n - 1 (u n can round up to n)
__device__ __forceinline__ int de_index(double u, int n) {
    const int k = (int)rn_mul(u, (double)n);
    return k < n - 1 ? k : n - 1;
}

// one workgroup per instance, one launch per generation
__global__ __launch_bounds__(WG) void de_step_kernel(DeState st, int g) {
    __shared__ double sPop[DE_MAX_POP];
    __shared__ double sVal[DE_MAX_NP], sRed[WG], sRow0[DE_MAX_DIM];
    __shared__ int sRedI[WG], sA[DE_MAX_NP], sB[DE_MAX_NP], sJ[DE_MAX_NP];
    __shared__ unsigned char sAcc[DE_MAX_NP];
    __shared__ double sF;
    const int r = blockIdx.x, tid = threadIdx.x, D = st.D, NP = st.NP, S = st.S, n = NP * D;
    const size_t m0 = (size_t)r * NP, x0 = m0 * D, tw = de_trace_row(D, NP);
    // the columns of a trace row
    const size_t oT = (size_t)1 + 3 * NP, oC = oT + n, oR = oC + n, oV = oR + n, oAc = oV + NP, oP = oAc + NP, oPv = oP + n,
                 oS = oPv + NP;
    double* row = st.trace ? st.trace + ((size_t)g * st.R + r) * tw : nullptr;      // generation g - 1 (g = 0: the start)
    const int code0 = g == 0 ? (int)DE_RAN : st.code[r];

    // ---- the population and its values into LDS
    {
        const double* px = g == 0 ? st.x0 + x0 : st.pop + x0;
        const double* pv = g == 0 ? st.f0 + m0 : st.val + m0;
        for (int e = tid; e < n; e += WG) {
            const double x = px[e];
            sPop[e] = x;
            if (g == 0) st.pop[x0 + e] = x;
        }
        for (int i = tid; i < NP; i += WG) {
            const double v = pv[i];
            sVal[i] = v;
            if (g == 0) st.val[m0 + i] = v;
        }
    }
    // ---- (a) select: member i takes its trial iff the trial's value is no NaN and (its own is NaN or trial >= own)
    unsigned word = 0;
    const bool select = g > 0 && code0 == DE_RAN;
    if (select) {
        for (int i = tid; i < NP; i += WG) {
            unsigned f = 0;
            const double tv = de_value(st, m0 + i, f), v = sVal[i];
            const bool acc = tv == tv && (v != v || tv >= v);
            word |= f | (tv == tv ? DE_W_TRIAL : 0u);
            sAcc[i] = acc ? 1 : 0;
            if (acc) {
                sVal[i] = tv;
                st.val[m0 + i] = tv;
            }
            if (row) {
                row[oV + i] = tv;
                row[oAc + i] = acc ? 1.0 : 0.0;
            }
        }
        __syncthreads();
        for (int e = tid; e < n; e += WG)
            if (sAcc[e / D]) {
                const double t = st.trial[x0 + e];
                sPop[e] = t;
                st.pop[x0 + e] = t;
            }
    } else if (row) {
        for (int i = tid; i < 2 * NP; i += WG) row[oV + i] = 0.0;
        if (g == 0)                                          // the start's row has no trials
            for (size_t e = tid; e < oV; e += WG) row[e] = 0.0;
    }
    // (lane tid looks at the members it wrote itself)
    for (int i = tid; i < NP; i += WG)
        if (!(fabs(sVal[i]) <= DE_DBL_MAX)) word |= DE_W_NOT_FINITE;
    __syncthreads();

    // ---- (b) the best member; SciPy's std <= atol + tol |mean| without the square root, asked behind a select only
    word = de_or(sRedI, word);
    const int best = de_best(sVal, sRed, sRedI, NP);
    const double sum = de_sum(sRed, NP, [&](int i) { return sVal[i]; });
    const double mean = rn_div(sum, (double)NP);
    const double m2 = de_sum(sRed, NP, [&](int i) {
        const double dv = rn_sub(sVal[i], mean);
        return rn_mul(dv, dv);
    });
    const double lim = rn_add(st.atol, rn_mul(st.tol, fabs(mean)));
    const bool converged = select && !(word & DE_W_NOT_FINITE) && m2 <= rn_mul((double)NP, rn_mul(lim, lim));
    const int code = code0 != DE_RAN ? (int)DE_STOPPED
                                     : (select && !(word & DE_W_TRIAL) ? (int)DE_ALL_NAN : (converged ? (int)DE_CONVERGED : (int)DE_RAN));
    if (tid == 0) {
        const unsigned fl = (word & DE_W_FLAGS) | (code != DE_RAN ? ROBO_FLAG_FROZEN : 0u);
        st.flags[r] = g == 0 ? fl : st.flags[r] | fl;
        st.best[r] = best;
        st.code[r] = code;
        if (g == 0) st.gen[r] = 0;
        else if (select) st.gen[r] = g;
    }
    if (row) {
        for (int e = tid; e < n; e += WG) row[oP + e] = sPop[e];
        for (int i = tid; i < NP; i += WG) row[oPv + i] = sVal[i];
        if (tid == 0) {
            row[oS] = (double)best;
            row[oS + 1] = sum;
            row[oS + 2] = mean;
            row[oS + 3] = m2;
            row[oS + 4] = (double)code;
        }
    }
    if (g >= st.T) return;

    // ---- (c) generation g's trials
    double* trow = row ? row + (size_t)st.R * tw : nullptr;
    const bool live = code == DE_RAN;
    const double* u = st.u ? st.u + ((size_t)g * st.R + r) * de_draws_row(D, NP) : nullptr;
    if (live) {
        if (tid == 0) {
            double uF, other;
            if (u) {
                uF = u[0];
            } else {
                unsigned c[4] = {(unsigned)g, (unsigned)r, 0xFFFFFFFFu, 0u};
                philox_uniform2(c, st.seed, uF, other);
            }
            sF = rn_add(st.f_lo, rn_mul(uF, rn_sub(st.f_hi, st.f_lo)));
        }
        for (int i = tid; i < NP; i += WG) {
            double ua, ub, uj, other;
            if (u) {
                const double* um = u + 1 + (size_t)i * (3 + 2 * D);
                ua = um[0];
                ub = um[1];
                uj = um[2];
            } else {
                unsigned c[4] = {(unsigned)g, (unsigned)r, (unsigned)i, 0u};
                philox_uniform2(c, st.seed, ua, ub);
                unsigned c1[4] = {(unsigned)g, (unsigned)r, (unsigned)i, 1u};
                philox_uniform2(c1, st.seed, uj, other);
            }
            int a = de_index(ua, NP - 1);
            a += a >= i ? 1 : 0;
            const int lo = a < i ? a : i, hi = a < i ? i : a;
            int b = de_index(ub, NP - 2);
            b += b >= lo ? 1 : 0;
            b += b >= hi ? 1 : 0;
            sA[i] = a;
            sB[i] = b;
            sJ[i] = de_index(uj, D);
        }
        __syncthreads();
        if (trow) {
            if (tid == 0) trow[0] = sF;
            for (int i = tid; i < NP; i += WG) {
                trow[1 + i] = (double)sA[i];
                trow[1 + NP + i] = (double)sB[i];
                trow[1 + 2 * NP + i] = (double)sJ[i];
            }
        }
    } else if (trow) {
        for (int i = tid; i < 1 + 3 * NP; i += WG) trow[i] = 0.0;
    }
    const double F = live ? sF : 0.0;
    for (int e = tid; e < n; e += WG) {
        const int i = e / D, d = e - i * D;
        double t = sPop[best * D + d];                       // a stopped instance hands copies of its best point to the solve
        bool cross = false, rep = false;
        if (live) {
            double uc;
            if (u) {
                uc = u[1 + (size_t)i * (3 + 2 * D) + 3 + d];
            } else {
                unsigned c[4] = {(unsigned)g, (unsigned)r, (unsigned)i, 2u + (unsigned)(d >> 1)};
                double p0, p1;
                philox_uniform2(c, st.seed, p0, p1);
                uc = (d & 1) ? p1 : p0;
            }
            cross = uc < st.cr || d == sJ[i];
            t = cross ? rn_add(t, rn_mul(F, rn_sub(sPop[sA[i] * D + d], sPop[sB[i] * D + d]))) : sPop[e];
            rep = !(t >= 0.0 && t <= 1.0);
            if (rep) {
                if (u) {
                    t = u[1 + (size_t)i * (3 + 2 * D) + 3 + D + d];
                } else {
                    unsigned c[4] = {(unsigned)g, (unsigned)r, (unsigned)i, 0x80000000u + (unsigned)(d >> 1)};
                    double p0, p1;
                    philox_uniform2(c, st.seed, p0, p1);
                    t = (d & 1) ? p1 : p0;
                }
            }
            st.trial[x0 + e] = t;
        }
        if (r == 0 && i == 0) sRow0[d] = t;
        for (int s = 0; s < S; ++s) st.model[s].Xcs[x0 + e] = t * st.model[s].ism[d];
        if (trow) {
            trow[oT + e] = t;
            trow[oC + e] = cross ? 1.0 : 0.0;
            trow[oR + e] = rep ? 1.0 : 0.0;
        }
    }
    if (r != 0) return;
    // rows of the handles beyond R NP replicate row 0, as scale_inputs_kernel's pad rows do
    __syncthreads();
    const long long first = (long long)st.R * n, last = st.m_pad * D;
    for (int s = 0; s < S; ++s) {
        double* X = st.model[s].Xcs;
        const double* ism = st.model[s].ism;
        for (long long e = first + tid; e < last; e += WG) X[e] = sRow0[e % D] * ism[e % D];
    }
}

// the best member of the instance with the largest best value, first on ties, NaN never -> st.out; the flag words of the
// candidate handle (the sweep's) and of the instances are reported, the handle's is cleared
__global__ void de_result_kernel(DeState st, unsigned* __restrict__ cand_flags) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int D = st.D, NP = st.NP;
    unsigned flags = *cand_flags;
    *cand_flags = 0u;
    int win = -1;
    double value = __longlong_as_double(0x7FF8000000000000LL);
    for (int r = 0; r < st.R; ++r) {
        flags |= st.flags[r];
        const double v = st.val[(size_t)r * NP + st.best[r]];
        if (v == v && (win < 0 || v > value)) {
            win = r;
            value = v;
        }
    }
    if (win < 0) flags |= ROBO_FLAG_NAN;
    const int w = win < 0 ? 0 : win;
    for (int d = 0; d < D; ++d) st.out[d] = st.pop[((size_t)w * NP + st.best[w]) * D + d];
    st.out[D] = value;
    st.out[D + 1] = __longlong_as_double((long long)win);
    st.out[D + 2] = __longlong_as_double((long long)flags);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
void de_free(DeWork* w) {
    if (!w) return;
    hipFree(w->d_block);
    hipFree(w->d_trace);
    delete w;
}

int launch_de_step(robo_ctx* ctx, const DeState& st, int g) {
    hipLaunchKernelGGL(de_step_kernel, dim3((unsigned)st.R), dim3(WG), 0, ctx->stream, st, g);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_de_result(robo_ctx* ctx, const DeState& st, unsigned* d_cand_flags) {
    hipLaunchKernelGGL(de_result_kernel, dim3(1), dim3(64), 0, ctx->stream, st, d_cand_flags);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

}  // namespace robo
