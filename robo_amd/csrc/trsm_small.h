// Pieces of the small-batch block-row step (predict.hip) that the chained form of the same step (trsm_chain.hip) shares:
// the LDS budget, the accumulator layout and the cross-covariance tile generated in registers.
#pragma once
#include "common.h"
#include "gemm_f64.h"
#include "kern_math.h"

namespace robo {

template <int MB, int DK> constexpr int small_stage() { return DK * (NB + 16 * MB) * LDS_LD; }   // DK x (L tile | V tile)
template <int MB, int DK> constexpr int small_smem_doubles() {   // T image + result image, or the two staging stages
    return 2 * MB * NB * 16 > 2 * small_stage<MB, DK>() ? 2 * MB * NB * 16 : 2 * small_stage<MB, DK>();
}

template <int MB>
struct AccS {
    v4d t[2][MB];   // [row block 2 wave + rbl][candidate block]
};

template <int KIND, int MB>
__device__ __forceinline__ void gen_cross_tile_s(const CovParams& cp, const double* __restrict__ Xc,
                                                 const double* __restrict__ Xt, int n_valid, double* smem,
                                                 AccS<MB>& acc) {
    constexpr int SC = 16 * MB, GD = 16, GXL = NB + 2, GCL = SC + 2;
    double* sX = smem;                 // [GD][GXL] training points
    double* sC = smem + GD * GXL;      // [GD][GCL] candidates
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, dim = cp.dim;
    const bool fab = KIND == ROBO_KERNEL_FABOLAS;
#pragma unroll
    for (int rbl = 0; rbl < 2; ++rbl)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) acc.t[rbl][mb] = fab ? v4d{1.0, 1.0, 1.0, 1.0} : v4d{0.0, 0.0, 0.0, 0.0};
    const int rbase = wave * 32 + (lane >> 4), cbase = lane & 15;
    for (int d0 = 0; d0 < dim; d0 += GD) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int idx = t + e * 256, row = idx >> 4, d = idx & 15;
            sX[d * GXL + row] = d0 + d < dim ? Xt[(size_t)row * dim + d0 + d] : 0.0;
        }
#pragma unroll
        for (int e = 0; e < MB; ++e) {
            const int idx = t + e * 256, row = idx >> 4, d = idx & 15;
            sC[d * GCL + row] = d0 + d < dim ? Xc[(size_t)row * dim + d0 + d] : 0.0;
        }
        __syncthreads();
        const int dn = dim - d0 < GD ? dim - d0 : GD;
        for (int d = 0; d < dn; ++d) {
            if (fab && d0 + d == dim - 1) break;
            double xi[MB];
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) xi[mb] = sC[d * GCL + cbase + mb * 16];
#pragma unroll
            for (int rbl = 0; rbl < 2; ++rbl)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double xj = sX[d * GXL + rbl * 16 + rbase + 4 * r];
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) {
                        const double df = xi[mb] - xj;
                        if (fab) acc.t[rbl][mb][r] *= matern52_1d(df);
                        else acc.t[rbl][mb][r] = fma(df, df, acc.t[rbl][mb][r]);
                    }
                }
        }
    }
    const int dl = (dim - 1) % GD;
#pragma unroll
    for (int rbl = 0; rbl < 2; ++rbl)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = rbl * 16 + rbase + 4 * r;
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                double uu = 0.0;
                if (fab) uu = sC[dl * GCL + cbase + mb * 16] * sX[dl * GXL + row];
                const double v = cov_finish<double, KIND>(cp, acc.t[rbl][mb][r], uu);
                acc.t[rbl][mb][r] = row < n_valid ? v : 0.0;
            }
        }
    __syncthreads();
}

}  // namespace robo
