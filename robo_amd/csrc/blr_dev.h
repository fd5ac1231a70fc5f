// Bayesian linear regression on basis features (blr.hip, api_blr.hip): the handle, what the host passes to the kernels and
// the one feature loader the statistics kernel and the candidate sweep share.  The rule is stated in include/robo_hip.h.
#pragma once
#include "common.h"
#include "gemm_f64.h"
#include "mlp_dev.h"

namespace robo {

constexpr int BLR_CHUNK = 1024;               // rows per workgroup of blr_stats_kernel: a constant of the code, so that the
                                              // order of every sum -- hence every bit of G, b, yy -- depends on n alone
constexpr int BLR_TC = 64;                    // candidates per workgroup of blr_sweep_kernel (16 per wave)
constexpr int BLR_XLD = ROBO_BLR_MAX_DIM + 1; // leading dimension of a staged tile of raw input rows
constexpr int BLR_EIG_LD = ROBO_BLR_MAX_FEATURES + 1;
constexpr int BLR_EIG_MAX_SWEEPS = 40;
constexpr double BLR_EPS = 2.220446049250313e-16;
constexpr double BLR_EIG_THRESHOLD = 4.0 * BLR_EPS;

// the feature map; FP = F rounded up to 16, 32, 64 or 128 (pad features are 0), DP = dim rounded up to 4
struct BlrFeat {
    int kind, dim, F, FP, DP;
    const double* omega;     // kind 3: DP x FP, pad rows and columns zero
    const double* phase;     // kind 3: FP
    double scale;
    MlpNet mlp;              // kind 4: the layer shape and the handle's own padded copy of the parameters (mlp_dev.h)
};
static_assert(BLR_XLD == MLP_LD, "mlp_features reads the staged rows of blr_stage_x");
inline int blr_row_width(const BlrFeat& ft) { return ft.kind == ROBO_BLR_FEAT_GIVEN ? ft.F : ft.dim; }
inline size_t blr_part_stride(int FP) { return (size_t)FP * FP + FP + 8; }   // [G | b | yy] of one chunk

// rows [row0, row0 + rows) of the caller's (limit x dim) inputs -> xs[r * BLR_XLD + d]; rows past `limit` and the
// coordinates dim .. DP - 1 are 0.  Kind 0 has no raw rows: nothing is staged.
__device__ __forceinline__ void blr_stage_x(const BlrFeat& ft, const double* __restrict__ src, long long row0, int rows,
                                            long long limit, double* xs) {
    if (ft.kind == ROBO_BLR_FEAT_GIVEN) return;
    for (int e = threadIdx.x; e < rows * ft.DP; e += WG) {
        const int r = e / ft.DP, d = e - r * ft.DP;
        xs[r * BLR_XLD + d] = (row0 + r < limit && d < ft.dim) ? src[(size_t)(row0 + r) * ft.dim + d] : 0.0;
    }
}

// phi(row0 + r)[f] -> dst[r * sr + f * sf] for r < rows (a multiple of 16), f < FP; rows past `limit` and features past F
// are 0.  Kinds 1 and 2 read the staged rows; kind 3 forms x . omega_f on the matrix pipe (one 16 x 16 tile of arguments
// per wave and step, coordinates in index order) and leaves scale cos(x . omega_f + phase_f); kind 0 copies the caller's
// row; kind 4 is the network's last hidden layer and a constant (mlp_features: barriers inside, so every thread of the
// workgroup reaches the loader).  A value depends on its own row alone.  Ends without a barrier.  NET says at compile time
// that the kind is 4: the kernels of kinds 0..3 are instantiated without the network's code and stay what they were.
template <bool NET>
__device__ __forceinline__ void blr_features(const BlrFeat& ft, const double* __restrict__ src, long long row0, int rows,
                                             long long limit, const double* xs, double* dst, int sr, int sf) {
    const int D = ft.dim, F = ft.F, FP = ft.FP;
    if constexpr (NET) {
        mlp_features(ft.mlp, row0, rows, limit, xs, dst, sr, sf, FP);
        return;
    }
    if (ft.kind == ROBO_BLR_FEAT_RFF) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nf = FP / 16, tiles = (rows / 16) * nf;
        for (int u = wave; u < tiles; u += WG / 64) {
            const int rt = u / nf, ft0 = (u - rt * nf) * 16;
            v4d acc = v4d{0.0, 0.0, 0.0, 0.0};
            for (int d0 = 0; d0 < ft.DP; d0 += 4)
                acc = mfma_f64(xs[(rt * 16 + (lane & 15)) * BLR_XLD + d0 + (lane >> 4)],
                               ft.omega[(size_t)(d0 + (lane >> 4)) * FP + ft0 + (lane & 15)], acc);
            const int f = ft0 + (lane & 15);
            const double ph = ft.phase[f];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = rt * 16 + (lane >> 4) + 4 * r;
                dst[row * sr + f * sf] = (row0 + row < limit && f < F) ? ft.scale * cos(acc[r] + ph) : 0.0;
            }
        }
        return;
    }
    for (int e = threadIdx.x; e < rows * FP; e += WG) {
        const int r = e / FP, f = e - r * FP;
        double v = 0.0;
        if (row0 + r < limit && f < F) {
            if (ft.kind == ROBO_BLR_FEAT_GIVEN) v = src[(size_t)(row0 + r) * F + f];
            else if (ft.kind == ROBO_BLR_FEAT_LINEAR) v = f < D ? xs[r * BLR_XLD + f] : 1.0;
            else v = f < D ? xs[r * BLR_XLD + f] * xs[r * BLR_XLD + f] : (f < 2 * D ? xs[r * BLR_XLD + f - D] : 1.0);
        }
        dst[r * sr + f * sf] = v;
    }
}

// ---- launchers (blr.hip; all asynchronous on ctx->stream) -----------------------------------------------------------------
// chunks [c0, c0 + nc) of the n rows -> nc partials [G | b | yy], blr_part_stride doubles each
int launch_blr_stats(robo_ctx* ctx, const BlrFeat& ft, const double* d_rows, const double* d_y, long long n, long long c0,
                     int nc, double* d_part);
// stats (+)= the nc partials, in chunk order
int launch_blr_sum(robo_ctx* ctx, const double* d_part, int nc, int FP, bool first, double* d_stats);
int launch_blr_eig(robo_ctx* ctx, const double* d_stats, int F, int FP, double* d_Qt, double* d_lam, double* d_c,
                   int* d_status);
int launch_blr_loglik(robo_ctx* ctx, const double* d_stats, const double* d_lam, const double* d_c, int F, int FP,
                      long long n, int S, const double* d_log_ab, int form, double* d_out);
int launch_blr_hypers(robo_ctx* ctx, const double* d_lam, const double* d_c, int F, int FP, int S, const double* d_ab,
                      double* d_wm, double* d_wv, double* d_invb);
int launch_blr_sweep(robo_ctx* ctx, const BlrFeat& ft, const double* d_rows, long long m, const double* d_Qt,
                     const double* d_wm, const double* d_wv, const double* d_invb, int S, double* d_mean, double* d_var,
                     double* d_per_sample);

}  // namespace robo

struct robo_blr {
    robo_ctx* ctx;
    robo::BlrFeat ft;            // (omega / phase point into d_feat)
    double* d_feat;              // kind 3: [omega (DP x FP) | phase (FP)]; kind 4: the padded parameters
    long long n;
    bool has_data, has_hypers;
    int S;
    double* d_rows;              // the uploaded training rows and targets: [X or Phi (n x width) | y (n)] (grows)
    size_t rows_cap;
    double* d_part;              // the chunk partials of one pass (grows)
    size_t part_cap;
    double* d_model;             // [G (FP x FP) | b (FP) | yy .. (8)] [Qt (FP x FP)] [lambda (FP)] [c (FP)]
    double *d_Qt, *d_lam, *d_c;
    int* d_status;               // [2]: the eigensolver's verdict (0 converged), its sweeps
    double* d_hyp;               // [alpha, beta (64 x 2)] [1 / beta (64)] [beta c / t (64 x FP)] [1 / t (64 x FP)]
    double *d_invb, *d_wm, *d_wv;
    double* d_ll;                // the likelihood call's [log alpha, log beta (S x 2) | out (S)] (grows)
    size_t ll_cap;
    double* d_cand;              // the uploaded candidate rows (grows)
    size_t cand_cap;
    double* d_ps;                // per-sample moments [means (S x m) | variances (S x m)] of a call that asks (grows)
    size_t ps_cap;
    robo_cand* k;                // the moments' tables and the acquisition's state, kept between calls of one m
};
