// Pathwise posterior samples (Matheron's rule; the rule is stated in include/robo_hip.h):
//
//   f_s(x) = c + sum_f phi_f(x) w_sf + sum_j k(x, X_j) alpha_sj
//
// One templated kernel, "two chained products with an element-wise middle".  A workgroup owns 64 rows of X and all paths;
// per tile of 64 rows of the other operand (training points, then features)
//
//   stage 1  t_ij = x_i . b_j                          the LDS-staged 4 x 4 micro-tiles of gram_tile.h, 16 dimensions per pass
//   middle   data:      amp k(|x_i|^2 + |X_j|^2 - 2 t_ij)   (cov_finish of kern_math.h, the dot form of pair_cov_dot)
//            features:  sqrt(2 amp / F) cos(t_ij + b_j)
//   stage 2  acc_is += middle_ij C_sj                   v_mfma_f64_16x16x4_f64; C (S_pad x N_pad resp. F_pad) row-major
//
// The middle tile goes from registers to LDS as the A operand of stage 2 and never to memory.  Wave w owns rows 16 w ..
// 16 w + 15 of the tile and every column tile of 16 paths: a path's accumulator sees the operand tiles in index order,
// k ascending inside the instruction, whatever its row's place in the batch and whatever the other paths are.  The middle's
// own arithmetic is rounded once per operation and never contracted (rn_*).  Pads: pad training rows and pad features
// meet zero weights, pad paths have zero weights everywhere, pad rows of X are neither stored nor reduced.
#include "paths.h"
#include "kern_math.h"

namespace robo {

constexpr int MID_DATA = 0, MID_FEAT = 1;

__device__ __forceinline__ double paths_nan() { return __longlong_as_double(0x7FF8000000000000LL); }

// (value, row) a beats b in a path's pick: np.argmax(-f) -- NaN maximal, the smaller value, the first index
__device__ __forceinline__ bool paths_better(double av, long long ai, double bv, long long bi) {
    if (ai < 0) return false;
    if (bi < 0) return true;
    const bool an = isnan(av), bn = isnan(bv);
    if (an || bn) return an && bn ? ai < bi : an;
    if (av != bv) return av < bv;
    return ai < bi;
}

// acc += middle(X[i0 .. i0 + 63] . B^T) C^T over `tiles` tiles of 64 rows of B (dim doubles each); C: 16 ns rows of ldc
// doubles.  sA: staging of stage 1 ([d][row], both operands), then the middle tile [row][col]; sC: the C tile; sN: the squared
// norms of the 64 rows of X, then of the 64 rows of B.  Ends on a barrier.
template <int MID, int KIND>
__device__ __forceinline__ void paths_pass(const PathsArgs& a, const double* __restrict__ B, const double* __restrict__ bias,
                                           int tiles, const double* __restrict__ C, int ldc, long long i0, double* sA,
                                           double* sC, double* sN, v4d (&acc)[4]) {
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4, dim = a.cp.dim;
    const int lane = t & 63, wave = t >> 6;
    double* sI = sA;
    double* sJ = sA + PD * PLD;
    for (int jt = 0; jt < tiles; ++jt) {
        const long long j0 = (long long)jt * PT;
        double dot[4][4];
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) dot[p][q] = 0.0;
        double nrm = 0.0;                   // threads 0..63: |x_i|^2 of row i0 + t; 64..127: |b_j|^2 of row j0 + t - 64
        const double* sMine = t < PT ? sI : sJ;
        for (int d0 = 0; d0 < dim; d0 += PD) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int idx = t + e * 256;
                const int row = idx >> 4, d = idx & 15;
                const bool ok = d0 + d < dim;
                sI[d * PLD + row] = ok ? a.X[(size_t)(i0 + row) * dim + d0 + d] : 0.0;
                sJ[d * PLD + row] = ok ? B[(size_t)(j0 + row) * dim + d0 + d] : 0.0;
            }
            __syncthreads();
            const int dn = dim - d0 < PD ? dim - d0 : PD;
            if (t < 2 * PT)
                for (int d = 0; d < dn; ++d) {
                    const double x = sMine[d * PLD + (t & (PT - 1))];
                    nrm = fma(x, x, nrm);
                }
            for (int d = 0; d < dn; ++d) {
                double xi[4], xj[4];
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    xi[p] = sI[d * PLD + ty * 4 + p];
                    xj[p] = sJ[d * PLD + tx * 4 + p];
                }
#pragma unroll
                for (int p = 0; p < 4; ++p)
#pragma unroll
                    for (int q = 0; q < 4; ++q) dot[p][q] = fma(xi[p], xj[q], dot[p][q]);
            }
            __syncthreads();
        }
        if (t < 2 * PT) sN[t] = nrm;
        for (int idx = t; idx < PATHS_SW * a.ns * PT; idx += 256) {
            const int s = idx >> 6, j = idx & (PT - 1);
            sC[s * PLD + j] = C[(size_t)s * ldc + j0 + j];
        }
        __syncthreads();
        // the middle: registers -> LDS, the A operand of stage 2 (over the staging buffers: every read of them is behind a barrier)
        double* sM = sA;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const double ni = sN[ty * 4 + p];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                double val;
                if (MID == MID_DATA) {
                    double r2 = rn_add(rn_add(ni, sN[PT + tx * 4 + q]), rn_mul(-2.0, dot[p][q]));
                    r2 = r2 < 0.0 ? 0.0 : r2;                                   // (a NaN stays)
                    if (a.self && i0 + ty * 4 + p == j0 + tx * 4 + q) r2 = 0.0;  // X against itself: the diagonal is exact
                    val = cov_finish<double, KIND>(a.cp, r2, 0.0);
                } else {
                    val = rn_mul(a.fscale, cos(rn_add(dot[p][q], bias[j0 + tx * 4 + q])));
                }
                sM[(ty * 4 + p) * PLD + tx * 4 + q] = val;
            }
        }
        __syncthreads();
        const double* pa = sM + (wave * 16 + (lane & 15)) * PLD + (lane >> 4);
        const double* pb = sC + (lane & 15) * PLD + (lane >> 4);
#pragma unroll 4
        for (int kk = 0; kk < PT / 4; ++kk) {
            const double av = pa[kk * 4];
#pragma unroll
            for (int tn = 0; tn < 4; ++tn)
                if (tn < a.ns) acc[tn] = mfma_f64(av, pb[tn * PATHS_SW * PLD + kk * 4], acc[tn]);
        }
        __syncthreads();
    }
}

template <int KIND>
__global__ __launch_bounds__(256, 2) void paths_kernel(PathsArgs a) {
    __shared__ double sA[PT * PLD];
    __shared__ double sC[PT * PLD];
    __shared__ double sN[2 * PT];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long i0 = a.c0 + (long long)blockIdx.x * PT;        // first row of X of this workgroup
    v4d acc[4];
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) acc[tn] = v4d{0.0, 0.0, 0.0, 0.0};
    paths_pass<MID_DATA, KIND>(a, a.Xs, nullptr, a.n_tiles, a.alpha, a.ld_alpha, i0, sA, sC, sN, acc);
    paths_pass<MID_FEAT, KIND>(a, a.omega, a.phase, a.f_tiles, a.w, a.ld_w, i0, sA, sC, sN, acc);
    // epilogue: + c, the output transform of post_kernel, NaN rows; transposed through LDS to [path][row]
    double* sV = sA;
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {
        if (tn >= a.ns) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = wave * 16 + (lane >> 4) + 4 * r, s = tn * PATHS_SW + (lane & 15);
            double f = acc[tn][r];
            if (!a.raw) {
                f = rn_add(f, a.mean_c);
                f = rn_add(rn_mul(f, a.y_std), a.y_mean);
            }
            if (isnan(sN[row])) f = paths_nan();                   // a NaN coordinate: NaN in every path
            sV[s * PLD + row] = f;
        }
    }
    __syncthreads();
    const long long left = a.m - i0;
    const int live = left >= PT ? PT : (left > 0 ? (int)left : 0);
    if (a.out)
        for (int idx = t; idx < a.S * PT; idx += 256) {
            const int s = idx >> 6, row = idx & (PT - 1);
            if (row < live) a.out[(size_t)s * a.ld_out + (size_t)(i0 - a.c0) + row] = sV[s * PLD + row];
        }
    if (a.raw || t >= a.S) return;
    double bv = 0.0;
    long long bi = -1;
    bool any_nan = false;
    for (int row = 0; row < live; ++row) {
        const double v = sV[t * PLD + row];
        any_nan = any_nan || isnan(v);
        if (paths_better(v, i0 + row, bv, bi)) {
            bv = v;
            bi = i0 + row;
        }
    }
    a.part_val[(size_t)t * a.n_part + (size_t)(i0 / PT)] = bv;
    a.part_idx[(size_t)t * a.n_part + (size_t)(i0 / PT)] = bi;
    if (any_nan) atomicOr(a.flags, (unsigned)ROBO_FLAG_NAN);
}

int launch_paths(robo_ctx* ctx, const PathsArgs& a, long long rows) {
    const dim3 grid((unsigned)(rows / PT));
    if (a.cp.kind == ROBO_KERNEL_MATERN52_ARD)
        hipLaunchKernelGGL((paths_kernel<ROBO_KERNEL_MATERN52_ARD>), grid, dim3(256), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL((paths_kernel<ROBO_KERNEL_RBF_ARD>), grid, dim3(256), 0, ctx->stream, a);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

// the winner of path blockIdx.x over its per-tile bests
__global__ __launch_bounds__(256) void paths_best_kernel(const double* __restrict__ part_val,
                                                         const long long* __restrict__ part_idx, long long n_part,
                                                         double* __restrict__ best_val, long long* __restrict__ best_idx) {
    __shared__ double sv[256];
    __shared__ long long si[256];
    const int t = threadIdx.x, s = blockIdx.x;
    double bv = 0.0;
    long long bi = -1;
    for (long long p = t; p < n_part; p += 256) {
        const double v = part_val[(size_t)s * n_part + p];
        const long long i = part_idx[(size_t)s * n_part + p];
        if (paths_better(v, i, bv, bi)) {
            bv = v;
            bi = i;
        }
    }
    sv[t] = bv;
    si[t] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o && paths_better(sv[t + o], si[t + o], sv[t], si[t])) {
            sv[t] = sv[t + o];
            si[t] = si[t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        best_val[s] = sv[0];
        best_idx[s] = si[0];
    }
}

int launch_paths_best(robo_ctx* ctx, const double* part_val, const long long* part_idx, long long n_part, int S, double* best_val,
                      long long* best_idx) {
    hipLaunchKernelGGL(paths_best_kernel, dim3(S), dim3(256), 0, ctx->stream, part_val, part_idx, n_part, best_val, best_idx);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

// r_s = (y - c) - Phi_X w_s - sd eps_s over the training rows, in place of Phi_X w_s; 0 in the pad rows
__global__ __launch_bounds__(256) void paths_rhs_kernel(double* __restrict__ r, const double* __restrict__ y,
                                                        const double* __restrict__ eps, int n, int n_pad, double mean_c,
                                                        double sd) {
    const int j = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (j >= n_pad) return;
    double v = 0.0;
    if (j < n) v = rn_sub(rn_sub(rn_sub(y[j], mean_c), r[(size_t)s * n_pad + j]), rn_mul(sd, eps[(size_t)s * n + j]));
    r[(size_t)s * n_pad + j] = v;
}

int launch_paths_rhs(robo_ctx* ctx, double* d_r, const double* d_y, const double* d_eps, int S, int n, int n_pad, double mean_c,
                     double sd) {
    hipLaunchKernelGGL(paths_rhs_kernel, dim3((unsigned)((n_pad + 255) / 256), S), dim3(256), 0, ctx->stream, d_r, d_y, d_eps, n,
                       n_pad, mean_c, sd);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

// rho_s = r_s - (K alpha_s + noise alpha_s) over the training rows, in place of K alpha_s; 0 in the pad rows
__global__ __launch_bounds__(256) void paths_residual_kernel(double* __restrict__ ka, const double* __restrict__ r,
                                                             const double* __restrict__ alpha, int n, int n_pad, double noise) {
    const int j = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (j >= n_pad) return;
    const size_t i = (size_t)s * n_pad + j;
    ka[i] = j < n ? rn_sub(rn_sub(r[i], ka[i]), rn_mul(noise, alpha[i])) : 0.0;
}

__global__ __launch_bounds__(256) void paths_add_kernel(double* __restrict__ alpha, const double* __restrict__ delta, int n_pad) {
    const int j = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (j >= n_pad) return;
    const size_t i = (size_t)s * n_pad + j;
    alpha[i] = rn_add(alpha[i], delta[i]);
}

int launch_paths_residual(robo_ctx* ctx, double* d_ka, const double* d_r, const double* d_alpha, int S, int n, int n_pad,
                          double noise) {
    hipLaunchKernelGGL(paths_residual_kernel, dim3((unsigned)((n_pad + 255) / 256), S), dim3(256), 0, ctx->stream, d_ka, d_r,
                       d_alpha, n, n_pad, noise);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_paths_add(robo_ctx* ctx, double* d_alpha, const double* d_delta, int S, int n_pad) {
    hipLaunchKernelGGL(paths_add_kernel, dim3((unsigned)((n_pad + 255) / 256), S), dim3(256), 0, ctx->stream, d_alpha, d_delta,
                       n_pad);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

// ---- alpha = L^-T L^-1 r over S right-hand sides: block rows of 128 with the fit's inverted diagonal blocks ------------------
// The recurrence of batch.hip's single right-hand side, with the path as the grid's second coordinate: a path's weights are
// formed by the same sequence of operations whatever S is.  Rows >= n (the augmented row, the padding) take no part.
//   forward, step i:   v_i = Linv_ii r_i ;  r_j -= L[j, i] v_i   for the block rows j > i   (one workgroup per j and path)
//   backward, step i:  a_i = Linv_ii^T v_i ;  v_j -= L[i, j]^T a_i   for the block columns j < i
// Every workgroup of a step forms the 128-entry diagonal solve itself; a launch boundary per step is the only ordering.
__global__ __launch_bounds__(256) void paths_fwd_kernel(const double* __restrict__ L, int ld, const double* __restrict__ Linv,
                                                        double* __restrict__ r_all, double* __restrict__ v_all, int i, int n) {
    __shared__ double sw[NB], sv[NB];
    double* r = r_all + (size_t)blockIdx.y * ld;
    double* v = v_all + (size_t)blockIdx.y * ld;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nv = n - i * NB < NB ? n - i * NB : NB;
    if (tid < NB) sw[tid] = tid < nv ? r[i * NB + tid] : 0.0;
    __syncthreads();
    const double* Li = Linv + (size_t)i * NB * NB;
    for (int row = wave * 32; row < wave * 32 + 32; ++row) {
        double a = 0.0;
        if (row < nv) {
            a = Li[row * NB + lane] * sw[lane];
            a = fma(Li[row * NB + 64 + lane], sw[64 + lane], a);
        }
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        if (lane == 0) sv[row] = a;
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid < NB) v[i * NB + tid] = sv[tid];
    const int jb = i + 1 + blockIdx.x;                      // the block row this workgroup updates
    if (jb * NB >= n) return;
    const double v0 = sv[lane], v1 = sv[64 + lane];
    for (int rr = wave * 32; rr < wave * 32 + 32; ++rr) {
        const int row = jb * NB + rr;
        double a = 0.0;
        if (row < n) {
            const double* Lr = L + (size_t)row * ld + (size_t)i * NB;
            a = Lr[lane] * v0;
            a = fma(Lr[64 + lane], v1, a);
        }
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        if (lane == 0 && row < n) r[row] -= a;
    }
}

__global__ __launch_bounds__(256) void paths_bwd_kernel(const double* __restrict__ L, int ld, const double* __restrict__ Linv,
                                                        double* __restrict__ v_all, double* __restrict__ a_all, int i, int n) {
    __shared__ double sv[NB], sb[NB], sp[NB];
    double* v = v_all + (size_t)blockIdx.y * ld;
    double* alpha = a_all + (size_t)blockIdx.y * ld;
    const int tid = threadIdx.x, c = tid & (NB - 1), half = tid >> 7;
    const int nv = n - i * NB < NB ? n - i * NB : NB;
    if (tid < NB) sv[tid] = tid < nv ? v[i * NB + tid] : 0.0;
    __syncthreads();
    const double* Li = Linv + (size_t)i * NB * NB;
    double a = 0.0;
    for (int row = half * 64; row < half * 64 + 64; ++row)
        if (row < nv && row >= c) a = fma(Li[row * NB + c], sv[row], a);
    if (half == 1) sp[c] = a;
    __syncthreads();
    if (half == 0) sb[c] = c < nv ? a + sp[c] : 0.0;
    __syncthreads();
    if (blockIdx.x == 0 && tid < NB) alpha[i * NB + tid] = sb[tid];
    const int jb = blockIdx.x;                              // the block column this workgroup updates
    if (jb >= i) return;
    a = 0.0;
    for (int row = half * 64; row < half * 64 + 64; ++row)
        if (row < nv) a = fma(L[(size_t)(i * NB + row) * ld + (size_t)jb * NB + c], sb[row], a);
    __syncthreads();
    if (half == 1) sp[c] = a;
    __syncthreads();
    if (half == 0) v[jb * NB + c] -= a + sp[c];
}

int launch_paths_solve(robo_ctx* ctx, const double* d_L, int n_pad, const double* d_Linv, int n, int S, double* d_r,
                       double* d_tmp) {
    const int nbk = (n + NB - 1) / NB;
    for (int i = 0; i < nbk; ++i)
        hipLaunchKernelGGL(paths_fwd_kernel, dim3((unsigned)(nbk - 1 - i > 1 ? nbk - 1 - i : 1), S), dim3(256), 0, ctx->stream,
                           d_L, n_pad, d_Linv, d_r, d_tmp, i, n);
    for (int i = nbk - 1; i >= 0; --i)
        hipLaunchKernelGGL(paths_bwd_kernel, dim3((unsigned)(i > 1 ? i : 1), S), dim3(256), 0, ctx->stream, d_L, n_pad, d_Linv,
                           d_tmp, d_r, i, n);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

}  // namespace robo
