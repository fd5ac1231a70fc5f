// Refinement of a path's minimiser by projected gradient descent, resident on the device (robo_paths_descend,
// robo_paths_refine_cand; the rule is stated in include/robo_hip.h):
//
//   f_s(x)       = (c + sum_f phi_f(x) w_sf + sum_j k(x~, X~_j) alpha_sj) y_std + y_mean
//   d f_s / d x_d = y_std ism_d [ sum_f (-fscale w_sf sin(x~ . omega_f + b_f)) omega_fd + sum_j (2 k'(r_j^2) alpha_sj) (x~_d - X~_jd) ]
//
// A path's value and gradient at a point need no solve and nothing but that point, so a descent never looks at another and
// ONE launch runs all of them from the evaluation of the starts to the last iteration: no launch per iteration, no grid-wide
// step.  A wave owns one descent; the PDG waves of a workgroup share every staged tile of 64 operand rows (training rows,
// then frequencies), whatever paths their descents are on: a path enters only through its weight row.  Per tile, lane l
//
//   stage 1   the differences x~_d - X~_jd (data) resp. the frequency omega_jd (features) of row j = 64 tile + l, kept in
//             registers, and their sum of squares r^2 resp. the dot product x~ . omega_j
//   middle    data:      k(r^2) through cov_finish of kern_math.h and 2 k'(r^2)
//             features:  fscale cos(. + b_j) and -fscale sin(. + b_j)
//   stage 2   one FMA into the value's accumulator and dim FMAs into the gradient's, each times the path's weight of row j
//
// so lane l accumulates rows l, 64 + l, ... of the training set and then of the features in index order, and the 64 lanes'
// sums meet in a butterfly (xor 32, 16, ..., 1; an addition commutes, so every lane ends with the same bits).  Nothing in
// that order depends on P, the slot, S, the other paths or the other descents of the workgroup.  Coordinates beyond dim up
// to the next multiple of 16 are staged as zeros and cost their FMAs.  The next tile's elements are loaded into registers
// before the current tile is consumed (an evaluation is a chain of (N + F) / 64 dependent tiles: without that every tile
// waited for its own loads; measured in NOTES.md "Refining a path's minimiser").  The decisions a host restatement must reproduce (the
// accept test, the step length, the projected unit step and its clip) are single rn_* operations on stored doubles.
#include "paths.h"
#include "kern_math.h"

namespace robo {

constexpr int DESC_DATA = 0, DESC_FEAT = 1;

__device__ __forceinline__ double refine_nan() { return __longlong_as_double(0x7FF8000000000000LL); }

// 2 amp f'(r2) of k = amp f(r2) (predgrad.hip): Matern-5/2 -amp (5/6)(1 + t) e^-t with t = sqrt(5 r2); RBF -k / 2
template <int KIND>
__device__ __forceinline__ double cov_slope2(const CovParams& cp, double r2, double k) {
    if (KIND == ROBO_KERNEL_MATERN52_ARD) {
        const double s = pos_sqrt(5.0 * r2);
        return -cp.amp * (5.0 / 3.0) * (1.0 + s) * exp_nonpos(-s);
    }
    return -k;
}

// One pass over `tiles` tiles of 64 rows of B (dim doubles each) for the PDG descents of the workgroup: facc += middle .
// weights, gacc += middle' . weights (x) rows.  sT: the staged tile [row][d], leading dimension 16 NCH + 1 (the lanes of a
// half wave read 32 distinct bank pairs); sYw: this wave's scaled trial point.  Ends on a barrier.
template <int MID, int KIND, int NCH>
__device__ __forceinline__ void descent_pass(const PathsDescentArgs& a, const double* __restrict__ B,
                                             const double* __restrict__ bias, const double* __restrict__ wrow, int rows,
                                             double* sT, const double* sYw, double& facc, double (&gacc)[NCH][16]) {
    constexpr int DP = 16 * NCH, LD = DP + 1, NE = PT * DP / (64 * PDG);
    const int t = threadIdx.x, lane = t & 63, D = a.cp.dim;
    const int tiles = (rows + PT - 1) / PT;
    // a thread's NE elements of the next tile wait in registers while the current one is consumed (up to 48 dimensions:
    // beyond, the differences and the accumulators of 64 coordinates leave no registers for them and they would spill)
    constexpr bool PRE = NCH < 4;
    double pre[PRE ? NE : 1];
    if constexpr (PRE) {
#pragma unroll
        for (int q = 0; q < NE; ++q) {
            const int e = t + q * 64 * PDG, row = e / DP, d = e % DP;
            pre[q] = (d < D && tiles > 0) ? B[(size_t)row * D + d] : 0.0;
        }
    }
    for (int jt = 0; jt < tiles; ++jt) {
        const int j0 = jt * PT, j = j0 + lane;
#pragma unroll
        for (int q = 0; q < NE; ++q) {
            const int e = t + q * 64 * PDG, row = e / DP, d = e % DP;
            if constexpr (PRE) sT[row * LD + d] = pre[q];
            else sT[row * LD + d] = d < D ? B[(size_t)(j0 + row) * D + d] : 0.0;
        }
        const bool live = j < rows;
        const double wt = live ? wrow[j] : 0.0;
        const double bj = (MID == DESC_FEAT && live) ? bias[j] : 0.0;
        if constexpr (PRE) {
            if (jt + 1 < tiles) {
#pragma unroll
                for (int q = 0; q < NE; ++q) {
                    const int e = t + q * 64 * PDG, row = e / DP, d = e % DP;
                    pre[q] = d < D ? B[(size_t)(j0 + PT + row) * D + d] : 0.0;
                }
            }
        }
        __syncthreads();
        double vec[NCH][16];
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const double b = sT[lane * LD + c * 16 + i], y = sYw[c * 16 + i];
                if (MID == DESC_DATA) {
                    const double df = y - b;
                    vec[c][i] = df;
                    acc = fma(df, df, acc);
                } else {
                    vec[c][i] = b;
                    acc = fma(y, b, acc);
                }
            }
        double vc, gc;
        if (MID == DESC_DATA) {
            vc = cov_finish<double, KIND>(a.cp, acc, 0.0);
            gc = cov_slope2<KIND>(a.cp, acc, vc);
        } else {
            const double arg = rn_add(acc, bj);
            vc = rn_mul(a.fscale, cos(arg));
            gc = -rn_mul(a.fscale, sin(arg));
        }
        if (!live) {                    // rows past the last one: no part in any sum, whatever the pad rows hold
            vc = 0.0;
            gc = 0.0;
        }
        facc = fma(vc, wt, facc);
        const double cj = gc * wt;
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int i = 0; i < 16; ++i) gacc[c][i] = fma(cj, vec[c][i], gacc[c][i]);
        __syncthreads();
    }
}

template <int KIND, int NCH>
__global__ __launch_bounds__(64 * PDG) void paths_descent_kernel(PathsDescentArgs a) {
    constexpr int DP = 16 * NCH, LD = DP + 1;
    __shared__ double sT[PT * LD];
    __shared__ double sY[PDG][DP];
    __shared__ int sActive[PDG];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, D = a.cp.dim;
    const int i = blockIdx.x * PDG + wave;
    const bool valid = i < a.P;
    const bool used = valid && (!a.start || a.start[i] >= 0);
    const int path = valid ? a.path_of[i] : 0;
    const bool mine = lane < D;                         // lane d carries coordinate d of the descent
    const size_t id = (size_t)(valid ? i : 0) * D + (mine ? lane : 0);
    const double ismd = mine ? a.ism[lane] : 0.0;
    const double* al = a.alpha + (size_t)path * a.ld_alpha;
    const double* wr = a.w + (size_t)path * a.ld_w;
    // the accepted point, its value and gradient; the pending trial; the step length and the one the trial was made with
    double xd = (used && mine) ? a.x0[id] : 0.0, gd = 0.0, yd = xd;
    double fx = refine_nan(), alpha = a.step0, aused = a.step0;
    int frozen = used ? 0 : 1, code = 2;

    for (int it = 0; it <= a.T; ++it) {
        const bool active = used && !frozen;
        if (lane < DP) sY[wave][lane] = mine ? rn_mul(yd, ismd) : 0.0;
        if (lane == 0) sActive[wave] = active ? 1 : 0;
        __syncthreads();
        int any = 0;
#pragma unroll
        for (int g = 0; g < PDG; ++g) any |= sActive[g];
        double fy = fx, gyd = gd;
        if (any) {                                       // (the same in every wave: the barriers of the passes are met by all)
            double facc = 0.0, gacc[NCH][16];
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int q = 0; q < 16; ++q) gacc[c][q] = 0.0;
            descent_pass<DESC_DATA, KIND, NCH>(a, a.Xs, nullptr, al, a.n, sT, sY[wave], facc, gacc);
            descent_pass<DESC_FEAT, KIND, NCH>(a, a.omega, a.phase, wr, a.F, sT, sY[wave], facc, gacc);
            for (int o = 32; o > 0; o >>= 1) facc += __shfl_xor(facc, o);
            double gsum = 0.0;
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    double v = gacc[c][q];
                    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
                    if (lane == c * 16 + q) gsum = v;
                }
            if (active) {
                fy = rn_add(rn_mul(rn_add(facc, a.mean_c), a.y_std), a.y_mean);
                gyd = rn_mul(rn_mul(gsum, ismd), a.y_std);
            }
        }

        // the decision (identical in every lane): robo_acq_refine_cand's, applied to -f
        const bool trial_bad = !isfinite(fy);
        const int was_frozen = frozen;
        const double alpha0 = alpha;
        bool accept = false;
        if (!used) {
            code = 2;
        } else if (it == 0) {            // the start itself: always the current point
            accept = true;
            code = trial_bad ? 3 : 1;
            if (trial_bad) frozen = 1;
        } else if (was_frozen) {
            code = 2;
        } else if (trial_bad) {          // value not finite: not taken, and the descent stops here
            code = 3;
            frozen = 1;
        } else {
            accept = fy < fx;
            code = accept ? 1 : 0;
            alpha = accept ? fmin(rn_mul(2.0, alpha0), 0.5) : rn_mul(alpha0, 0.5);
        }
        if (a.trace && valid) {
            double* row = a.trace + ((size_t)it * a.P + i) * (2 * D + 3);
            if (mine) {
                row[lane] = yd;
                row[D + 1 + lane] = gyd;
            }
            if (lane == 0) {
                row[D] = fy;
                row[2 * D + 1] = aused;
                row[2 * D + 2] = (double)code;
            }
        }
        if (accept) {
            xd = yd;
            gd = gyd;
            fx = fy;
        }
        // next trial: the projected direction of unit length against the gradient, clipped to the box
        const double gp = (mine && !((xd <= 0.0 && gd > 0.0) || (xd >= 1.0 && gd < 0.0))) ? gd : 0.0;
        double n2 = 0.0;
        for (int d = 0; d < D; ++d) {
            const double v = __shfl(gp, d);
            n2 = rn_add(n2, rn_mul(v, v));
        }
        const double nrm = sqrt(n2);
        const bool more = it < a.T;
        if (used && more && !frozen && !(nrm > 0.0 && isfinite(nrm))) frozen = 1;     // no descent direction left inside the box
        double yn = xd;
        if (more && !frozen) {
            yn = rn_sub(xd, rn_div(rn_mul(alpha, gp), nrm));
            yn = yn < 0.0 ? 0.0 : (yn > 1.0 ? 1.0 : yn);
        }
        yd = yn;
        aused = alpha;
        if (used && frozen && !was_frozen && lane == 0) atomicOr(a.flags, (unsigned)ROBO_FLAG_FROZEN);
        __syncthreads();                                 // sY and sActive are rewritten by the next iteration
    }
    if (!valid) return;
    if (mine) {
        a.x[id] = xd;
        a.g[id] = gd;
    }
    if (lane == 0) {
        a.f[i] = fx;
        a.code[i] = code;
    }
}

template <int KIND>
static void launch_descent_kind(robo_ctx* ctx, const PathsDescentArgs& a) {
    const dim3 grid((unsigned)((a.P + PDG - 1) / PDG)), block(64 * PDG);
    switch ((a.cp.dim + 15) / 16) {
    case 1: hipLaunchKernelGGL((paths_descent_kernel<KIND, 1>), grid, block, 0, ctx->stream, a); break;
    case 2: hipLaunchKernelGGL((paths_descent_kernel<KIND, 2>), grid, block, 0, ctx->stream, a); break;
    case 3: hipLaunchKernelGGL((paths_descent_kernel<KIND, 3>), grid, block, 0, ctx->stream, a); break;
    default: hipLaunchKernelGGL((paths_descent_kernel<KIND, 4>), grid, block, 0, ctx->stream, a); break;
    }
}

int launch_paths_descent(robo_ctx* ctx, const PathsDescentArgs& a) {
    if (a.cp.kind == ROBO_KERNEL_MATERN52_ARD) launch_descent_kind<ROBO_KERNEL_MATERN52_ARD>(ctx, a);
    else launch_descent_kind<ROBO_KERNEL_RBF_ARD>(ctx, a);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

// ---- the starts of the fused form: per path the n_starts smallest group bests of the sweep ------------------------------------
// The sweep left, per path, the best row of every group of 64 consecutive candidates (part_val / part_idx: first index on
// ties, NaN maximal, row -1 for a group without a live row).  A group is eligible unless its best is NaN or its row -1.
// Order: ascending value, ties by ascending row (= ascending group), -0 read as +0.  One workgroup per path: the 96-bit key
// (order-preserving bits of the value, group number) of the n_starts-th smallest group is found digit by digit, 8 bits per
// pass, from integer counts; the groups up to that key are collected in arrival order and placed by rank counting, a
// permutation because the keys are distinct.  The result is a function of the values alone.
constexpr int STARTS_PASSES = 12;
constexpr int STARTS_MAX = 1024;             // ROBO_PATHS_MAX_STARTS

__device__ __forceinline__ unsigned long long starts_key(double v) {
    const long long b = __double_as_longlong(v == 0.0 ? 0.0 : v);
    const unsigned long long u = (unsigned long long)b;
    return b < 0 ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ unsigned starts_digit(unsigned long long hi, unsigned lo, int pass) {
    return pass < 8 ? (unsigned)(hi >> (56 - 8 * pass)) & 255u : (lo >> (24 - 8 * (pass - 8))) & 255u;
}
__device__ __forceinline__ bool starts_prefix(unsigned long long hi, unsigned lo, unsigned long long thi, unsigned tlo, int pass) {
    if (pass == 0) return true;
    if (pass < 8) return (hi >> (64 - 8 * pass)) == (thi >> (64 - 8 * pass));
    if (hi != thi) return false;
    if (pass == 8) return true;
    return (lo >> (32 - 8 * (pass - 8))) == (tlo >> (32 - 8 * (pass - 8)));
}

__global__ __launch_bounds__(256) void paths_starts_kernel(const double* __restrict__ part_val,
                                                           const long long* __restrict__ part_idx, long long n_part, int K,
                                                           const double* __restrict__ Xc, int D, PathsRefineState st) {
    __shared__ unsigned hist[256];
    __shared__ unsigned long long thi;
    __shared__ unsigned tlo, remaining, keff, count;
    __shared__ double cval[STARTS_MAX];
    __shared__ long long crow[STARTS_MAX], srow[STARTS_MAX];
    const int t = threadIdx.x, s = blockIdx.x;
    const double* pv = part_val + (size_t)s * n_part;
    const long long* pi = part_idx + (size_t)s * n_part;
    if (t == 0) {
        thi = 0ull;
        tlo = 0u;
        remaining = 0u;
        keff = 0u;
        count = 0u;
    }
    for (int pass = 0; pass < STARTS_PASSES; ++pass) {
        hist[t] = 0u;
        __syncthreads();
        if (pass == 0 || remaining > 0u)
            for (long long p = t; p < n_part; p += 256) {
                const double v = pv[p];
                if (v != v || pi[p] < 0) continue;
                const unsigned long long hi = starts_key(v);
                if (starts_prefix(hi, (unsigned)p, thi, tlo, pass)) atomicAdd(&hist[starts_digit(hi, (unsigned)p, pass)], 1u);
            }
        __syncthreads();
        if (t == 0) {
            if (pass == 0) {
                unsigned long long total = 0;
                for (int d = 0; d < 256; ++d) total += hist[d];
                keff = total < (unsigned long long)K ? (unsigned)total : (unsigned)K;
                remaining = keff;
            }
            if (remaining > 0u) {
                unsigned below = 0u;
                int digit = 255;
                for (int d = 0; d < 256; ++d) {
                    const unsigned c = hist[d];
                    if (below + c >= remaining) {
                        digit = d;
                        break;
                    }
                    below += c;
                }
                remaining -= below;
                if (pass < 8) thi |= (unsigned long long)digit << (56 - 8 * pass);
                else tlo |= (unsigned)digit << (24 - 8 * (pass - 8));
            }
        }
        __syncthreads();
    }
    const int ke = (int)keff;
    if (ke > 0)
        for (long long p = t; p < n_part; p += 256) {
            const double v = pv[p];
            if (v != v || pi[p] < 0) continue;
            const unsigned long long hi = starts_key(v);
            if (hi < thi || (hi == thi && (unsigned)p <= tlo)) {
                const unsigned slot = atomicAdd(&count, 1u);
                if (slot < (unsigned)STARTS_MAX) {
                    cval[slot] = v;
                    crow[slot] = pi[p];
                }
            }
        }
    __syncthreads();
    double* sval = st.sval + (size_t)s * K;
    long long* start = st.start + (size_t)s * K;
    for (int i = t; i < K; i += 256) {
        st.path_of[(size_t)s * K + i] = s;
        if (i >= ke) {
            srow[i] = -1;
            start[i] = -1;
            sval[i] = refine_nan();
            continue;
        }
        const unsigned long long hi = starts_key(cval[i]);
        int rank = 0;
        for (int j = 0; j < ke; ++j) {
            const unsigned long long hj = starts_key(cval[j]);
            rank += (hj < hi || (hj == hi && crow[j] < crow[i])) ? 1 : 0;
        }
        srow[rank] = crow[i];
        start[rank] = crow[i];
        sval[rank] = cval[i];
    }
    __syncthreads();
    for (int e = t; e < K * D; e += 256) {
        const int i = e / D, d = e - i * D;
        st.x0[((size_t)s * K + i) * D + d] = srow[i] >= 0 ? Xc[(size_t)srow[i] * D + d] : 0.0;
    }
}

int launch_paths_starts(robo_ctx* ctx, const double* part_val, const long long* part_idx, long long n_part, int S, int n_starts,
                        const double* Xc, int dim, const PathsRefineState& st) {
    hipLaunchKernelGGL(paths_starts_kernel, dim3(S), dim3(256), 0, ctx->stream, part_val, part_idx, n_part, n_starts, Xc, dim,
                       st);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

// ---- the winners -------------------------------------------------------------------------------------------------------------------
// Thread s: among the used slots of path s the descent with the smallest final value, first slot on ties, NaN only if
// nothing else is there -> res[s] = (point, value, the row its start came from); no used slot: (0, NaN, -1).  sweep_only
// (no steps were asked for): the first start -- the sweep's own pick -- with the value the sweep computed for it.
__global__ __launch_bounds__(64) void paths_winners_kernel(int S, int K, int D, PathsRefineState st, int sweep_only,
                                                           unsigned* __restrict__ flags) {
    const int s = threadIdx.x;
    if (s >= S) return;
    const size_t s0 = (size_t)s * K;
    int best = -1;
    for (int k = 0; k < K; ++k) {
        if (st.start[s0 + k] < 0) continue;
        if (best < 0) {
            best = k;
            if (sweep_only) break;
            continue;
        }
        const double a = st.f[s0 + k], b = st.f[s0 + best];
        if ((b != b && a == a) || a < b) best = k;
    }
    double* res = st.res + (size_t)s * (D + 2);
    const double* x = sweep_only ? st.x0 : st.x;
    for (int d = 0; d < D; ++d) res[d] = best >= 0 ? x[(s0 + best) * D + d] : 0.0;
    const double value = best >= 0 ? (sweep_only ? st.sval[s0 + best] : st.f[s0 + best]) : refine_nan();
    if (value != value) atomicOr(flags, (unsigned)ROBO_FLAG_NAN);
    res[D] = value;
    res[D + 1] = __longlong_as_double(best >= 0 ? st.start[s0 + best] : -1LL);
}

int launch_paths_winners(robo_ctx* ctx, int S, int n_starts, int dim, const PathsRefineState& st, bool sweep_only,
                         unsigned* flags) {
    hipLaunchKernelGGL(paths_winners_kernel, dim3(1), dim3(64), 0, ctx->stream, S, n_starts, dim, st, sweep_only ? 1 : 0, flags);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

}  // namespace robo
