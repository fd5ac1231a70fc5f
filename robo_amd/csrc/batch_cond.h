// The tile loop of the conditioning passes (batch.hip batch_cond_kernel, qei.hip qei_cond_kernel): k_*(x)^T beta of 64
// candidates against every tile of 128 training points, stated once.
// A workgroup of 256 owns 64 candidates, one per lane; its four waves split every tile (32 rows each, staged as
// [dimension][row]: all lanes of a wave read the same word, a broadcast).  A lane keeps its candidate's scaled coordinates
// in registers while dim <= 16 (SMALLD) and re-reads them per chunk of 16 dimensions otherwise.  Per pair the covariance is
// accumulated dimension by dimension with direct differences, as the cross-gram generators of predict.hip do, and
// multiplied into the lane's running sum.  The four partial sums are added in wave order by cond_join.
#pragma once
#include "common.h"
#include "kern_math.h"

namespace robo {

constexpr int BC_CAND = 64;          // candidates per workgroup of a conditioning pass (one per lane; the 4 waves split the rows)
constexpr int BC_ROWS = 32;          // training rows per wave and tile
constexpr int BC_LD = NB + 2;

// this wave's share of k_*(x_ii)^T beta; sX [16 * BC_LD] and sB [NB] are the workgroup's staging arrays; every thread of
// the workgroup calls it
template <int KIND, bool SMALLD>
__device__ __forceinline__ double cond_kstar_dot(const double* __restrict__ Xc, const double* __restrict__ Xs,
                                                 const double* __restrict__ ism, const CovParams& cp, int n,
                                                 const double* __restrict__ beta, long long ii, double* sX, double* sB) {
    const int tid = threadIdx.x, wave = tid >> 6, D = cp.dim;
    double xc[16];
    if (SMALLD) {
#pragma unroll
        for (int d = 0; d < 16; ++d) xc[d] = d < D ? Xc[ii * D + d] * ism[d] : 0.0;
    }
    const int nbk = (n + NB - 1) / NB;
    double dot = 0.0;
    for (int tile = 0; tile < nbk; ++tile) {
        double acc[BC_ROWS], uu[BC_ROWS];
#pragma unroll
        for (int r = 0; r < BC_ROWS; ++r) cov_init<double, KIND>(cp, acc[r], uu[r]);
        for (int d0 = 0; d0 < D; d0 += 16) {
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int idx = tid + e * 256, row = idx >> 4, d = idx & 15;
                const int rg = tile * NB + row;
                sX[d * BC_LD + row] = (d0 + d < D && rg < n) ? Xs[(size_t)rg * D + d0 + d] : 0.0;
            }
            if (d0 == 0 && tid < NB) sB[tid] = tile * NB + tid < n ? beta[tile * NB + tid] : 0.0;
            __syncthreads();
            const int dn = D - d0 < 16 ? D - d0 : 16;
            const double* sx = sX + wave * BC_ROWS;
            if (SMALLD) {
#pragma unroll
                for (int d = 0; d < 16; ++d) {
                    if (d < dn) {
#pragma unroll
                        for (int r = 0; r < BC_ROWS; ++r)
                            cov_step<double, KIND>(cp, d, xc[d], sx[d * BC_LD + r], acc[r], uu[r]);
                    }
                }
            } else {
                for (int d = 0; d < dn; ++d) {
                    const double xi = Xc[ii * D + d0 + d] * ism[d0 + d];
#pragma unroll
                    for (int r = 0; r < BC_ROWS; ++r)
                        cov_step<double, KIND>(cp, d0 + d, xi, sx[d * BC_LD + r], acc[r], uu[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < BC_ROWS; ++r)
            dot = fma(cov_finish<double, KIND>(cp, acc[r], uu[r]), sB[wave * BC_ROWS + r], dot);
    }
    return dot;
}

// c(x_i) = k(x_i, x_j) - k_*(x_i)^T beta - sum_{t < nt} c_t(x_i) c_t(x_j) / d_t: the covariance of x_i and the pick x_j (its
// scaled coordinates in sJ) under the real data, then under the nt earlier conditioning steps as well, whose c_t and d_t
// are kept:  cov_t+1(x, x') = cov_t(x, x') - c_t(x) c_t(x') / d_t
template <int KIND>
__device__ __forceinline__ double cond_cov(const double* __restrict__ Xc, const double* __restrict__ ism, const CovParams& cp,
                                           const double* sJ, double ktb, long long i, long long pj, int nt,
                                           const double* __restrict__ chist, const double* __restrict__ dhist,
                                           long long m_pad) {
    double a0, u0;
    cov_init<double, KIND>(cp, a0, u0);
    for (int d = 0; d < cp.dim; ++d) cov_step<double, KIND>(cp, d, Xc[i * cp.dim + d] * ism[d], sJ[d], a0, u0);
    double c = cov_finish<double, KIND>(cp, a0, u0) - ktb;
    for (int t = 0; t < nt; ++t) {
        const double* ct = chist + (size_t)t * m_pad;
        c -= ct[i] * (ct[pj] / dhist[t]);
    }
    return c;
}

}  // namespace robo
