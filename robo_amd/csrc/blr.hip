// Bayesian linear regression on basis features: the kernels (the rule is stated in include/robo_hip.h, the layout in
// DESIGN.md).
//   blr_stats_kernel    one workgroup per chunk of BLR_CHUNK rows: the feature tile of 16 rows is formed in LDS by
//                       blr_features (blr_dev.h) as [feature][row], the operand layout of gemm_f64.h, and Phi^T Phi is
//                       accumulated on v_mfma_f64_16x16x4_f64 with the SAME tile as both operands; Phi^T y and y^T y
//                       ride along on the vector pipe.  One barrier per tile (two feature stages, two row stages).
//   blr_sum_kernel      the chunk partials added in chunk order, one thread per entry: no atomics anywhere
//   blr_eig_kernel      two-sided cyclic Jacobi in one workgroup, G in LDS, Q^T in memory (rows p, q of Q^T are what a
//                       rotation touches: coalesced), round-robin pairs
//   blr_loglik_kernel   one lane per (alpha, beta)
//   blr_hypers_kernel   the per-sample weight tables beta c_j / t_sj and 1 / t_sj of the sweep
//   blr_sweep_kernel    64 candidates per workgroup: features by the same loader, psi = Q^T phi on the matrix pipe with Q^T
//                       streamed through LDS in 16-column stages, psi kept in LDS, then the fold over the samples
#include <cmath>

#include "blr_dev.h"

namespace robo {

// ---- G = Phi^T Phi, b = Phi^T y, yy = y^T y per chunk -------------------------------------------------------------------------
// NT = FP / 16.  The four waves own the quadrants of the FP x FP tile grid (NT = 1: wave 0 alone owns the one tile).
template <int NT, bool NET>
__global__ __launch_bounds__(WG) void blr_stats_kernel(BlrFeat ft, const double* __restrict__ rows,
                                                       const double* __restrict__ y, long long n, long long c0,
                                                       double* __restrict__ part) {
    constexpr int FP = 16 * NT, H = NT >= 2 ? NT / 2 : 1;
    __shared__ double sphi[2][FP * LDS_LD];
    __shared__ double sx[2][BK * BLR_XLD];
    __shared__ double sy[3][BK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wy = wave >> 1, wx = wave & 1;
    const bool live = NT >= 2 || wave == 0;
    const long long beg = (c0 + blockIdx.x) * BLR_CHUNK;
    const long long end = beg + BLR_CHUNK < n ? beg + BLR_CHUNK : n;
    const int tiles = (int)((end - beg + BK - 1) / BK);
    v4d acc[H][H];
#pragma unroll
    for (int i = 0; i < H; ++i)
#pragma unroll
        for (int j = 0; j < H; ++j) acc[i][j] = v4d{0.0, 0.0, 0.0, 0.0};
    double side = 0.0;       // thread f < FP: b_f; thread WG - 1: yy

    blr_stage_x(ft, rows, beg, BK, end, sx[0]);
    if (tid < BK) sy[0][tid] = beg + tid < end ? y[beg + tid] : 0.0;
    __syncthreads();
    for (int t = 0; t < tiles; ++t) {
        const long long r0 = beg + (long long)t * BK;
        if (t + 1 < tiles) {
            blr_stage_x(ft, rows, r0 + BK, BK, end, sx[(t + 1) & 1]);
            if (tid < BK) sy[(t + 1) % 3][tid] = r0 + BK + tid < end ? y[r0 + BK + tid] : 0.0;
        }
        double* cur = sphi[t & 1];
        blr_features<NET>(ft, rows, r0, BK, end, sx[t & 1], cur, 1, LDS_LD);
        __syncthreads();
        if (live) {
            const double* pa = cur + (wy * H * 16 + (lane & 15)) * LDS_LD + (lane >> 4);
            const double* pb = cur + (wx * H * 16 + (lane & 15)) * LDS_LD + (lane >> 4);
#pragma unroll
            for (int kk = 0; kk < BK / 4; ++kk) {
                double a[H], b[H];
#pragma unroll
                for (int i = 0; i < H; ++i) {
                    a[i] = pa[i * 16 * LDS_LD + kk * 4];
                    b[i] = pb[i * 16 * LDS_LD + kk * 4];
                }
#pragma unroll
                for (int i = 0; i < H; ++i)
#pragma unroll
                    for (int j = 0; j < H; ++j) acc[i][j] = mfma_f64(a[i], b[j], acc[i][j]);
            }
        }
        const double* ty = sy[t % 3];
        if (tid < FP) {
#pragma unroll
            for (int k = 0; k < BK; ++k) side = fma(cur[tid * LDS_LD + k], ty[k], side);
        } else if (tid == WG - 1) {
#pragma unroll
            for (int k = 0; k < BK; ++k) side = fma(ty[k], ty[k], side);
        }
    }
    double* out = part + (size_t)blockIdx.x * (FP * FP + FP + 8);
    if (live) {
#pragma unroll
        for (int i = 0; i < H; ++i)
#pragma unroll
            for (int j = 0; j < H; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    out[((wy * H + i) * 16 + (lane >> 4) + 4 * r) * FP + (wx * H + j) * 16 + (lane & 15)] = acc[i][j][r];
    }
    if (tid < FP) out[FP * FP + tid] = side;
    else if (tid == WG - 1) out[FP * FP + FP] = side;
}

__global__ __launch_bounds__(WG) void blr_sum_kernel(const double* __restrict__ part, int nc, int stride, int len, int first,
                                                     double* __restrict__ stats) {
    const int e = blockIdx.x * WG + threadIdx.x;
    if (e >= len) return;
    double s = first ? 0.0 : stats[e];
    for (int c = 0; c < nc; ++c) s += part[(size_t)c * stride + e];
    stats[e] = s;
}

// ---- G = Q diag(lambda) Q^T ------------------------------------------------------------------------------------------------
// Round r of a sweep pairs the players 0 .. M - 1 (M = F rounded up to even; a pair with player F is idle) by the circle
// method: M / 2 disjoint rotations, computed by M / 2 threads from the diagonal and applied by all of them, first to the
// columns, then to the rows of G and to the rows of Q^T.  A pair counts as rotated away when
//     |g_pq| <= BLR_EIG_THRESHOLD max(sqrt(|g_pp g_qq|), eps trace(G)):
// the floor eps trace(G) lets a rank-deficient G, whose null space carries diagonal entries of either sign at rounding
// level, converge; it costs nothing normwise.
__global__ __launch_bounds__(WG) void blr_eig_kernel(const double* __restrict__ stats, int F, int FP, double* __restrict__ Qt,
                                                     double* __restrict__ lam, double* __restrict__ cvec,
                                                     int* __restrict__ status) {
    __shared__ double G[ROBO_BLR_MAX_FEATURES * BLR_EIG_LD];
    __shared__ double s_cs[ROBO_BLR_MAX_FEATURES / 2][2];
    __shared__ int s_pq[ROBO_BLR_MAX_FEATURES / 2][2];
    __shared__ double s_red[WG];
    __shared__ double s_floor, s_off;
    const int tid = threadIdx.x;
    for (int e = tid; e < F * F; e += WG) G[(e / F) * BLR_EIG_LD + e % F] = stats[(e / F) * FP + e % F];
    for (int e = tid; e < FP * FP; e += WG) Qt[e] = (e / FP == e % FP && e / FP < F) ? 1.0 : 0.0;
    __syncthreads();
    if (tid == 0) {
        double tr = 0.0;
        for (int i = 0; i < F; ++i) tr += fabs(G[i * BLR_EIG_LD + i]);
        s_floor = tr * BLR_EPS;
        // a NaN or an infinity in feature f of any row is in g_ff, one in any target is in yy: both sums of squares
        s_off = tr + stats[FP * FP + FP];
    }
    __syncthreads();
    if (!(fabs(s_off) <= 1.79769313486231570e308)) {             // (uniform: every thread reads the same word)
        if (tid == 0) {
            status[0] = 2;
            status[1] = 0;
        }
        return;
    }
    const int M = (F + 1) / 2 * 2, np = M / 2, rounds = M - 1;
    int sweep = 0, converged = 0;
    for (; sweep < BLR_EIG_MAX_SWEEPS && !converged; ++sweep) {
        double off = 0.0;
        for (int r = 0; r < rounds; ++r) {
            if (tid < np) {
                int a = (r + tid) % (M - 1), b = tid == 0 ? M - 1 : (r - tid + (M - 1)) % (M - 1);
                const int p = a < b ? a : b, q = a < b ? b : a;
                double c = 1.0, s = 0.0;
                if (q < F) {
                    const double gpp = G[p * BLR_EIG_LD + p], gqq = G[q * BLR_EIG_LD + q], gpq = G[p * BLR_EIG_LD + q];
                    if (gpq != 0.0) {
                        const double ratio = fabs(gpq) / fmax(sqrt(fabs(gpp * gqq)), s_floor);
                        off = fmax(off, ratio);
                        if (!(ratio <= BLR_EIG_THRESHOLD)) {
                            const double tau = (gqq - gpp) / (2.0 * gpq);
                            const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                            c = 1.0 / sqrt(1.0 + t * t);
                            s = t * c;
                        }
                    }
                }
                s_pq[tid][0] = p;
                s_pq[tid][1] = q;
                s_cs[tid][0] = c;
                s_cs[tid][1] = s;
            }
            __syncthreads();
            for (int e = tid; e < np * F; e += WG) {             // G <- G J: columns p, q
                const int pr = e / F, i = e - pr * F;
                const double c = s_cs[pr][0], s = s_cs[pr][1];
                if (s == 0.0) continue;
                const int p = s_pq[pr][0], q = s_pq[pr][1];
                const double a = G[i * BLR_EIG_LD + p], b = G[i * BLR_EIG_LD + q];
                G[i * BLR_EIG_LD + p] = c * a - s * b;
                G[i * BLR_EIG_LD + q] = s * a + c * b;
            }
            __syncthreads();
            for (int e = tid; e < np * F; e += WG) {             // G <- J^T G: rows p, q; Q^T likewise
                const int pr = e / F, j = e - pr * F;
                const double c = s_cs[pr][0], s = s_cs[pr][1];
                if (s == 0.0) continue;
                const int p = s_pq[pr][0], q = s_pq[pr][1];
                const double a = G[p * BLR_EIG_LD + j], b = G[q * BLR_EIG_LD + j];
                G[p * BLR_EIG_LD + j] = j == q ? 0.0 : c * a - s * b;
                G[q * BLR_EIG_LD + j] = j == p ? 0.0 : s * a + c * b;
                const double u = Qt[p * FP + j], v = Qt[q * FP + j];
                Qt[p * FP + j] = c * u - s * v;
                Qt[q * FP + j] = s * u + c * v;
            }
            __syncthreads();
        }
        s_red[tid] = off;
        __syncthreads();
        if (tid == 0) {
            double m = 0.0;
            for (int i = 0; i < np; ++i) m = fmax(m, s_red[i]);
            s_off = m;
        }
        __syncthreads();
        converged = s_off <= BLR_EIG_THRESHOLD;
    }
    if (tid < FP) {
        double l = 0.0, c = 0.0;
        if (tid < F) {
            l = fmax(G[tid * BLR_EIG_LD + tid], 0.0);
            for (int i = 0; i < F; ++i) c = fma(Qt[tid * FP + i], stats[FP * FP + i], c);
        }
        lam[tid] = l;
        cvec[tid] = c;
    }
    if (tid == 0) {
        status[0] = converged ? 0 : 1;
        status[1] = sweep;
    }
}

// ---- S marginal log-likelihoods -----------------------------------------------------------------------------------------
// t_j = beta lambda_j + alpha;  |y - Phi m|^2 = yy - beta sum_j c_j^2 (beta lambda_j + 2 alpha) / t_j^2 (the two sums of the
// expansion taken together), clamped at 0;  m^T m = beta^2 sum_j c_j^2 / t_j^2;  log det A = sum_j log t_j
__global__ __launch_bounds__(WG) void blr_loglik_kernel(const double* __restrict__ stats, const double* __restrict__ lam,
                                                        const double* __restrict__ cvec, int F, int FP, double n, int S,
                                                        const double* __restrict__ log_ab, int form,
                                                        double* __restrict__ out) {
    const int s = blockIdx.x * WG + threadIdx.x;
    if (s >= S) return;
    const double la = log_ab[2 * s], lb = log_ab[2 * s + 1], alpha = exp(la), beta = exp(lb), yy = stats[FP * FP + FP];
    double fit = 0.0, mm = 0.0, logdet = 0.0;
    for (int j = 0; j < F; ++j) {
        const double t = beta * lam[j] + alpha, w = cvec[j] / t, w2 = w * w;
        fit += w2 * (beta * lam[j] + 2.0 * alpha);
        mm += w2;
        logdet += log(t);
    }
    mm *= beta * beta;
    const double res2 = fmax(yy - beta * fit, 0.0);
    double mll = 0.5 * F * la + 0.5 * n * lb - 0.5 * n * 1.8378770664093453;      // log(2 pi)
    mll -= 0.5 * beta * (form == 0 ? sqrt(res2) : res2);
    mll -= 0.5 * alpha * mm;
    mll -= 0.5 * logdet;
    out[s] = mll;
}

__global__ __launch_bounds__(WG) void blr_hypers_kernel(const double* __restrict__ lam, const double* __restrict__ cvec, int F,
                                                        int FP, int S, const double* __restrict__ ab, double* __restrict__ wm,
                                                        double* __restrict__ wv, double* __restrict__ invb) {
    const int e = blockIdx.x * WG + threadIdx.x;
    if (e >= S * FP) return;
    const int s = e / FP, j = e - s * FP;
    const double alpha = ab[2 * s], beta = ab[2 * s + 1], t = beta * lam[j] + alpha;
    wm[e] = j < F ? beta * cvec[j] / t : 0.0;
    wv[e] = j < F ? 1.0 / t : 0.0;
    if (j == 0) invb[s] = 1.0 / beta;
}

// ---- the candidate sweep -----------------------------------------------------------------------------------------------------
// Wave w owns candidates 16 w .. 16 w + 15 of the tile and all NT column tiles of psi = phi Q (contraction in index order, 16
// features per stage of Q^T).  The fold: thread (candidate, group g) takes the samples g, g + 4, .. with the features in index
// order; the mixture adds the four groups' sums in group order.  Nothing a candidate's values are made of depends on its
// row, on m or on the other candidates.
template <int NT, bool NET>
__global__ __launch_bounds__(WG) void blr_sweep_kernel(BlrFeat ft, const double* __restrict__ rows, long long m,
                                                       const double* __restrict__ Qt, const double* __restrict__ wm,
                                                       const double* __restrict__ wv, const double* __restrict__ invb, int S,
                                                       double* __restrict__ out_mean, double* __restrict__ out_var,
                                                       double* __restrict__ out_ps) {
    constexpr int FP = 16 * NT, PLD = FP + 1, SQ = ROBO_BLR_MAX_SAMPLES / 4;
    __shared__ double sp[BLR_TC * PLD];
    __shared__ double sq[2][FP * LDS_LD];
    __shared__ double sx[BLR_TC * BLR_XLD];
    __shared__ double s_pm[4][BLR_TC], s_pv[4][BLR_TC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = (long long)blockIdx.x * BLR_TC;
    blr_stage_x(ft, rows, row0, BLR_TC, m, sx);
    Tile4 rq = tile_load_regs<FP>(Qt, FP, 0);
    tile_store_lds<FP>(sq[0], rq);
    __syncthreads();
    blr_features<NET>(ft, rows, row0, BLR_TC, m, sx, sp, PLD, 1);
    __syncthreads();
    v4d acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = v4d{0.0, 0.0, 0.0, 0.0};
    for (int kt = 0; kt < NT; ++kt) {
        const bool more = kt + 1 < NT;
        if (more) rq = tile_load_regs<FP>(Qt, FP, (kt + 1) * BK);
        const double* pa = sp + (wave * 16 + (lane & 15)) * PLD + kt * BK + (lane >> 4);
        const double* pb = sq[kt & 1] + (lane & 15) * LDS_LD + (lane >> 4);
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
            const double a = pa[kk * 4];
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[j] = mfma_f64(a, pb[j * 16 * LDS_LD + kk * 4], acc[j]);
        }
        if (more) tile_store_lds<FP>(sq[(kt + 1) & 1], rq);
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) sp[(wave * 16 + (lane >> 4) + 4 * r) * PLD + j * 16 + (lane & 15)] = acc[j][r];
    __syncthreads();

    const int cand = lane, g = wave;
    const long long row = row0 + cand;
    double am[SQ], av[SQ];
#pragma unroll
    for (int q = 0; q < SQ; ++q) am[q] = av[q] = 0.0;
    for (int j = 0; j < ft.F; ++j) {
        const double psi = sp[cand * PLD + j], psi2 = psi * psi;
#pragma unroll
        for (int q = 0; q < SQ; ++q) {
            const int s = g + 4 * q;
            if (s < S) {
                am[q] = fma(psi, wm[s * FP + j], am[q]);
                av[q] = fma(psi2, wv[s * FP + j], av[q]);
            }
        }
    }
    double sum_m = 0.0, sum_v = 0.0;
#pragma unroll
    for (int q = 0; q < SQ; ++q) {
        const int s = g + 4 * q;
        if (s < S) {
            const double v = av[q] + invb[s];
            sum_m += am[q];
            sum_v += v;
            if (out_ps && row < m) {
                out_ps[(size_t)s * m + row] = am[q];
                out_ps[(size_t)(S + s) * m + row] = v;
            }
        }
    }
    s_pm[g][cand] = sum_m;
    s_pv[g][cand] = sum_v;
    __syncthreads();
    if (g == 0 && row < m) {
        const double mean = (((s_pm[0][cand] + s_pm[1][cand]) + s_pm[2][cand]) + s_pm[3][cand]) / (double)S;
        const double var = (((s_pv[0][cand] + s_pv[1][cand]) + s_pv[2][cand]) + s_pv[3][cand]) / (double)S;
        out_mean[row] = mean;
        out_var[row] = var < BLR_EPS ? BLR_EPS : var;          // (a NaN stays a NaN)
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
#define BLR_BY_NT(FP, ...)             \
    switch ((FP) / 16) {               \
        case 1: { constexpr int NT = 1; __VA_ARGS__; } break; \
        case 2: { constexpr int NT = 2; __VA_ARGS__; } break; \
        case 4: { constexpr int NT = 4; __VA_ARGS__; } break; \
        default: { constexpr int NT = 8; __VA_ARGS__; } break; \
    }
// NET: feature kind 4, the only instantiations that hold the network's loader and take its dynamic LDS
#define BLR_BY_KIND(FT, ...)                                                       \
    if ((FT).kind == ROBO_BLR_FEAT_MLP) {                                          \
        constexpr bool NET = true;                                                 \
        constexpr size_t LDS = MLP_ACT_BYTES;                                      \
        BLR_BY_NT((FT).FP, __VA_ARGS__)                                            \
    } else {                                                                       \
        constexpr bool NET = false;                                                \
        constexpr size_t LDS = 0;                                                  \
        BLR_BY_NT((FT).FP, __VA_ARGS__)                                            \
    }

int launch_blr_stats(robo_ctx* ctx, const BlrFeat& ft, const double* d_rows, const double* d_y, long long n, long long c0,
                     int nc, double* d_part) {
    BLR_BY_KIND(ft, hipLaunchKernelGGL(HIP_KERNEL_NAME(blr_stats_kernel<NT, NET>), dim3(nc), dim3(WG), LDS, ctx->stream, ft,
                                       d_rows, d_y, n, c0, d_part));
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_blr_sum(robo_ctx* ctx, const double* d_part, int nc, int FP, bool first, double* d_stats) {
    const int len = FP * FP + FP + 1;
    hipLaunchKernelGGL(blr_sum_kernel, dim3((len + WG - 1) / WG), dim3(WG), 0, ctx->stream, d_part, nc,
                       (int)blr_part_stride(FP), len, first ? 1 : 0, d_stats);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_blr_eig(robo_ctx* ctx, const double* d_stats, int F, int FP, double* d_Qt, double* d_lam, double* d_c,
                   int* d_status) {
    hipLaunchKernelGGL(blr_eig_kernel, dim3(1), dim3(WG), 0, ctx->stream, d_stats, F, FP, d_Qt, d_lam, d_c, d_status);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_blr_loglik(robo_ctx* ctx, const double* d_stats, const double* d_lam, const double* d_c, int F, int FP,
                      long long n, int S, const double* d_log_ab, int form, double* d_out) {
    hipLaunchKernelGGL(blr_loglik_kernel, dim3((S + WG - 1) / WG), dim3(WG), 0, ctx->stream, d_stats, d_lam, d_c, F, FP,
                       (double)n, S, d_log_ab, form, d_out);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_blr_hypers(robo_ctx* ctx, const double* d_lam, const double* d_c, int F, int FP, int S, const double* d_ab,
                      double* d_wm, double* d_wv, double* d_invb) {
    hipLaunchKernelGGL(blr_hypers_kernel, dim3((S * FP + WG - 1) / WG), dim3(WG), 0, ctx->stream, d_lam, d_c, F, FP, S, d_ab,
                       d_wm, d_wv, d_invb);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_blr_sweep(robo_ctx* ctx, const BlrFeat& ft, const double* d_rows, long long m, const double* d_Qt,
                     const double* d_wm, const double* d_wv, const double* d_invb, int S, double* d_mean, double* d_var,
                     double* d_per_sample) {
    const unsigned blocks = (unsigned)((m + BLR_TC - 1) / BLR_TC);
    BLR_BY_KIND(ft, hipLaunchKernelGGL(HIP_KERNEL_NAME(blr_sweep_kernel<NT, NET>), dim3(blocks), dim3(WG), LDS, ctx->stream, ft,
                                       d_rows, m, d_Qt, d_wm, d_wv, d_invb, S, d_mean, d_var, d_per_sample));
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

}  // namespace robo
