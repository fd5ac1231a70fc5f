// A small tanh network trained on the device (mlp.hip, api_mlp.hip) and evaluated inside the feature loader of the Bayesian
// linear regression (blr_dev.h, feature kind 4): the handle, the two parameter layouts and the device functions the kernels
// share.  The rule is stated in include/robo_hip.h.
//
// The PACKED layout (the C ABI's, P doubles): per hidden layer l = 1 .. L   W_l (in_l x H, row-major, W[i][j] = input i ->
// unit j; in_1 = dim, in_l = H), then b_l (H); then w_out (H), b_out (1).  Adam's moments and the gradient share it.
// The PADDED layout (what the loader and the forward kernel read, straight from L2 as matrix-instruction operands): per
// layer W_l (KP_l x HP; KP_1 = DP = dim rounded up to 4, KP_l = HP = H rounded up to 16), then b_l (HP); then w_out (HP),
// b_out (1).  Every pad entry is 0, so a pad unit is tanh(0) = 0 and feeds nothing.
#pragma once
#include "common.h"

namespace robo {

constexpr int MLP_MAX = 64;                   // the cap on dim and on the width (ROBO_MLP_MAX_DIM, ROBO_MLP_MAX_WIDTH)
constexpr int MLP_LD = MLP_MAX + 1;           // leading dimension of every LDS tile of weights, rows or activations: the
                                              // transposed fragment reads of the backward pass then touch 16 distinct banks
constexpr int MLP_TR = 16;                    // rows per tile of the gradient kernel
constexpr int MLP_MAX_PASS = 1024;            // chunk partials in memory at a time, whatever the workspace
// the dynamic LDS a kernel that calls mlp_features is launched with: two activation tiles.  Dynamic, so that the statistics
// kernel and the sweep carry it for feature kind 4 alone and the other kinds keep their LDS footprint and occupancy.
constexpr size_t MLP_ACT_BYTES = 2 * MLP_TR * MLP_LD * sizeof(double);

struct MlpNet {
    int dim, L, H, DP, IP, HP, P;             // IP = dim rounded up to 16 (the tile rows of dW_1)
    const double* pad;                        // the padded parameters
};
__host__ __device__ inline int mlp_in(const MlpNet& s, int l) { return l == 0 ? s.dim : s.H; }          // l = 0 .. L - 1
__host__ __device__ inline int mlp_w_off(const MlpNet& s, int l) {
    return l == 0 ? 0 : (s.dim + 1) * s.H + (l - 1) * (s.H + 1) * s.H;
}
__host__ __device__ inline int mlp_b_off(const MlpNet& s, int l) { return mlp_w_off(s, l) + mlp_in(s, l) * s.H; }
__host__ __device__ inline int mlp_out_off(const MlpNet& s) { return mlp_w_off(s, s.L); }             // w_out; b_out at P - 1
__host__ __device__ inline int mlp_kp(const MlpNet& s, int l) { return l == 0 ? s.DP : s.HP; }
__host__ __device__ inline int mlp_pad_off(const MlpNet& s, int l) {
    return l == 0 ? 0 : (s.DP + 1) * s.HP + (l - 1) * (s.HP + 1) * s.HP;
}
__host__ __device__ inline int mlp_pad_len(const MlpNet& s) { return mlp_pad_off(s, s.L) + s.HP + 1; }
// entry e of the packed layout is a weight (decayed by l2), not a bias
__host__ __device__ inline bool mlp_is_weight(const MlpNet& s, int e) {
    if (e >= mlp_out_off(s)) return e < s.P - 1;
    const int first = (s.dim + 1) * s.H;
    if (e < first) return e < s.dim * s.H;
    return (e - first) % ((s.H + 1) * s.H) < s.H * s.H;
}

// one 16 x 16 tile of  A (16 rows, K columns, leading dimension lda) . W (K rows, leading dimension ldw)[:, col0 .. col0 + 15]
// by one wave, the contraction in index order, four coordinates per instruction
__device__ __forceinline__ v4d mlp_tile(const double* a, int lda, const double* W, int ldw, int K, int col0) {
    const int lane = threadIdx.x & 63;
    v4d acc = v4d{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < K; k0 += 4)
        acc = mfma_f64(a[(lane & 15) * lda + k0 + (lane >> 4)], W[(size_t)(k0 + (lane >> 4)) * ldw + col0 + (lane & 15)], acc);
    return acc;
}

// phi(row0 + r)[f] = [a_L (H), 1] -> dst[r * sr + f * sf] for r < rows (a multiple of 16), f < FP; rows past `limit` and
// features past H are 0.  xs: the staged raw rows (leading dimension MLP_LD, coordinates dim .. DP - 1 zero).  Sixteen rows at
// a time: layer 1 as the random Fourier branch forms x . omega (staged rows against weight fragments from L2), the further
// layers through an LDS activation tile, tanh applied when a tile is written.  Every thread of the workgroup must call it
// (barriers inside when L > 1); a value depends on its own row alone.  Ends without a barrier.  The kernel is launched with MLP_ACT_BYTES of dynamic LDS.
__device__ __forceinline__ void mlp_features(const MlpNet& s, long long row0, int rows, long long limit, const double* xs,
                                             double* dst, int sr, int sf, int FP) {
    HIP_DYNAMIC_SHARED(double, s_act)                            // [2][MLP_TR * MLP_LD]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nt = s.HP / 16;
    for (int sub = 0; sub < rows / 16; ++sub) {
        if (sub > 0 && s.L > 1) __syncthreads();                 // the previous sixteen rows' last layer has read its tile
        const double* in = xs + sub * 16 * MLP_LD;
        for (int l = 0; l < s.L; ++l) {
            const double* W = s.pad + mlp_pad_off(s, l);
            const double* bias = W + mlp_kp(s, l) * s.HP;
            const bool last = l == s.L - 1;
            for (int u = wave; u < nt; u += WG / 64) {
                const v4d acc = mlp_tile(in, MLP_LD, W, s.HP, mlp_kp(s, l), u * 16);
                const int f = u * 16 + (lane & 15);
                const double b = bias[f];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = (lane >> 4) + 4 * r, grow = sub * 16 + row;
                    const double v = tanh(acc[r] + b);
                    if (!last) s_act[(l & 1) * MLP_TR * MLP_LD + row * MLP_LD + f] = v;
                    else dst[grow * sr + f * sf] = row0 + grow < limit ? (f < s.H ? v : f == s.H ? 1.0 : 0.0) : 0.0;
                }
            }
            if (!last) __syncthreads();
            in = s_act + (l & 1) * MLP_TR * MLP_LD;
        }
    }
    const int extra = FP - s.HP;                                  // the constant feature when H is a multiple of 16, and the pad
    for (int e = threadIdx.x; e < rows * extra; e += WG) {
        const int r = e / extra, f = s.HP + e - r * extra;
        dst[r * sr + f * sf] = (row0 + r < limit && f == s.H) ? 1.0 : 0.0;
    }
}

// ---- the gradient of a tile of 16 rows, shared by the full-batch trainer (mlp.hip) and the SGHMC chains (bnn.hip) -------------
// the LDS of a gradient workgroup: 3 x 64 x 65 weights (99 840 bytes), four activation tiles and two delta tiles of 16 x 65
// (49 920), the biases, the output layer and the tile's targets and errors: 154 248 bytes (150.6 KiB) of gfx950's 160 KiB
struct MlpLds {
    double W[3][MLP_MAX * MLP_LD];
    double act[4][MLP_TR * MLP_LD];
    double del[2][MLP_TR * MLP_LD];
    double b[3][MLP_MAX];
    double wout[MLP_MAX];
    double y[MLP_TR], err[MLP_TR], sq[MLP_TR];
    double red[WG];
    double bout;
};

// the packed parameters -> LDS, pad rows and columns zero
__device__ __forceinline__ void mlp_stage_weights(const MlpNet& s, const double* p, MlpLds& m) {
    const int tid = threadIdx.x;
    for (int l = 0; l < s.L; ++l) {
        const int in = mlp_in(s, l), kp = l == 0 ? s.IP : s.HP;
        const double* W = p + mlp_w_off(s, l);
        for (int e = tid; e < kp * s.HP; e += WG) {
            const int i = e / s.HP, j = e - i * s.HP;
            m.W[l][i * MLP_LD + j] = (i < in && j < s.H) ? W[i * s.H + j] : 0.0;
        }
        if (tid < s.HP) m.b[l][tid] = tid < s.H ? p[mlp_b_off(s, l) + tid] : 0.0;
    }
    if (tid < s.HP) m.wout[tid] = tid < s.H ? p[mlp_out_off(s) + tid] : 0.0;
    if (tid == 0) m.bout = p[s.P - 1];
    __syncthreads();
}

// A workgroup's gradient sums, in registers across the tiles of its rows.  acc[l][i][j]: the wave (wy, wx) = (wave >> 1,
// wave & 1) owns tile (I, J) = (wy hi + i, wx hj + j) of dW_l's grid of 16 x 16 tiles (hi, hj: half the grid's rows and
// columns, rounded up), lane and register r of it entry (16 I + (lane >> 4) + 4 r, 16 J + (lane & 15)) -- the matrix
// instruction's accumulator map.  gb[l]: thread j < HP holds d / d b_l[j].  side: thread 64 + j holds d / d w_out[j], thread
// 128 d / d b_out, thread 129 the sum of the squared errors.
struct MlpGrad {
    v4d acc[3][2][2];
    double gb[3];
    double side;
};
__device__ __forceinline__ void mlp_grad_zero(MlpGrad& G) {
#pragma unroll
    for (int l = 0; l < 3; ++l) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) G.acc[l][i][j] = v4d{0.0, 0.0, 0.0, 0.0};
        G.gb[l] = 0.0;
    }
    G.side = 0.0;
}
// the tile a wave owns at (l, i, j) -> its place (I, J) in dW_l's grid; false: the wave owns none there
__device__ __forceinline__ bool mlp_owned_tile(const MlpNet& s, int l, int i, int j, int& I, int& J) {
    const int wave = threadIdx.x >> 6, nt = s.HP / 16, it = (l == 0 ? s.IP : s.HP) / 16, hi = (it + 1) / 2, hj = (nt + 1) / 2;
    I = (wave >> 1) * hi + i;
    J = (wave & 1) * hj + j;
    return i < hi && j < hj && I < it && J < nt;
}

// G += the gradient of  sum_r (f(x_r) - y_r)^2 c1 / (2 c2)  over the tile's rows r0 .. min(r0 + 16, end) - 1: the error that
// goes back is (c1 (f - y)) / c2.  Row r is rows[r] (idx == nullptr) or rows[idx[r]].  The weights are in LDS
// (mlp_stage_weights).  Every thread of the workgroup calls it; ends on a barrier behind which no thread reads the weights.
__device__ __forceinline__ void mlp_tile_grad(const MlpNet& s, MlpLds& m, const double* __restrict__ rows,
                                              const double* __restrict__ y, const int* idx, long long r0, long long end,
                                              double c1, double c2, MlpGrad& G) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = s.L, H = s.H, HP = s.HP, nt = HP / 16;
    for (int e = tid; e < MLP_TR * s.IP; e += WG) {
        const int r = e / s.IP, d = e - r * s.IP;
        double v = 0.0;
        if (r0 + r < end && d < s.dim) v = rows[(size_t)(idx ? (long long)idx[r0 + r] : r0 + r) * s.dim + d];
        m.act[0][r * MLP_LD + d] = v;
    }
    if (tid < MLP_TR) m.y[tid] = r0 + tid < end ? y[idx ? (long long)idx[r0 + tid] : r0 + tid] : 0.0;
    __syncthreads();
    for (int l = 0; l < L; ++l) {                                        // a_(l+1) = tanh(a_l W_l + b_l)
        for (int u = wave; u < nt; u += WG / 64) {
            const v4d z = mlp_tile(m.act[l], MLP_LD, m.W[l], MLP_LD, l == 0 ? s.DP : HP, u * 16);
            const int f = u * 16 + (lane & 15);
            const double b = m.b[l][f];
#pragma unroll
            for (int r = 0; r < 4; ++r) m.act[l + 1][((lane >> 4) + 4 * r) * MLP_LD + f] = tanh(z[r] + b);
        }
        __syncthreads();
    }
    if (tid < MLP_TR) {                                                  // f = a_L . w_out + b_out, units in index order
        double f = m.bout;
        for (int j = 0; j < H; ++j) f = fma(m.act[L][tid * MLP_LD + j], m.wout[j], f);
        const double e = r0 + tid < end ? f - m.y[tid] : 0.0;
        m.err[tid] = (c1 * e) / c2;
        m.sq[tid] = e * e;
    }
    __syncthreads();
    double* dl = m.del[L & 1];                                           // delta_L = err  w_out (1 - a_L^2)
    for (int e = tid; e < MLP_TR * HP; e += WG) {
        const int r = e / HP, j = e - r * HP;
        const double a = m.act[L][r * MLP_LD + j];
        dl[r * MLP_LD + j] = (m.err[r] * m.wout[j]) * (1.0 - a * a);
    }
    if (tid >= 64 && tid < 64 + H) {
        for (int r = 0; r < MLP_TR; ++r) G.side = fma(m.err[r], m.act[L][r * MLP_LD + tid - 64], G.side);
    } else if (tid == 128) {
        for (int r = 0; r < MLP_TR; ++r) G.side = G.side + m.err[r];
    } else if (tid == 129) {
        for (int r = 0; r < MLP_TR; ++r) G.side = G.side + m.sq[r];
    }
    __syncthreads();
#pragma unroll
    for (int l = 2; l >= 0; --l) {                                       // (unrolled: acc and gb stay in registers)
        if (l >= L) continue;
        const double* dcur = m.del[(l + 1) & 1];
        const double* aprev = m.act[l];
#pragma unroll
        for (int i = 0; i < 2; ++i)                                      // dW_l += a_l^T delta_(l+1): the wave's quadrant
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                int I, J;
                if (mlp_owned_tile(s, l, i, j, I, J)) {
#pragma unroll
                    for (int k0 = 0; k0 < MLP_TR; k0 += 4)
                        G.acc[l][i][j] = mfma_f64(aprev[(k0 + (lane >> 4)) * MLP_LD + I * 16 + (lane & 15)],
                                                  dcur[(k0 + (lane >> 4)) * MLP_LD + J * 16 + (lane & 15)], G.acc[l][i][j]);
                }
            }
        if (tid < HP) {
            double g = G.gb[l];
            for (int r = 0; r < MLP_TR; ++r) g = g + dcur[r * MLP_LD + tid];
            G.gb[l] = g;
        }
        if (l > 0) {                                                     // delta_l = (delta_(l+1) W_l^T) (1 - a_l^2)
            double* dnext = m.del[l & 1];
            for (int u = wave; u < nt; u += WG / 64) {
                v4d z = v4d{0.0, 0.0, 0.0, 0.0};
                for (int k0 = 0; k0 < HP; k0 += 4)
                    z = mfma_f64(dcur[(lane & 15) * MLP_LD + k0 + (lane >> 4)],
                                 m.W[l][(u * 16 + (lane & 15)) * MLP_LD + k0 + (lane >> 4)], z);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int e = ((lane >> 4) + 4 * r) * MLP_LD + u * 16 + (lane & 15);
                    const double a = aprev[e];
                    dnext[e] = z[r] * (1.0 - a * a);
                }
            }
        }
        __syncthreads();
    }
}

// entry e of the padded layout from the packed parameters p
__device__ __forceinline__ double mlp_pad_entry(const MlpNet& s, const double* __restrict__ p, int e) {
    const int tail = mlp_pad_off(s, s.L);
    if (e >= tail) {
        const int j = e - tail;
        return j == s.HP ? p[s.P - 1] : (j < s.H ? p[mlp_out_off(s) + j] : 0.0);
    }
    int l = 0;
    while (l + 1 < s.L && e >= mlp_pad_off(s, l + 1)) ++l;
    const int o = e - mlp_pad_off(s, l), kp = mlp_kp(s, l), i = o / s.HP, j = o - i * s.HP;
    if (j < s.H) {
        if (i < mlp_in(s, l)) return p[mlp_w_off(s, l) + i * s.H + j];
        if (i == kp) return p[mlp_b_off(s, l) + j];
    }
    return 0.0;
}

// ---- launchers (mlp.hip; all asynchronous on ctx->stream) ---------------------------------------------------------------------
struct MlpTrain {                 // what one training call passes to its kernels; every pointer device memory
    MlpNet net;
    double *params, *mom;         // P; [m (P) | v (P)]
    double* keep;                 // [params | m | v] before the last update (a diverged run is put back from it)
    const double *rows, *y;       // n x dim, n
    long long n;
    double* part;                 // the chunk partials of one pass, P + 1 doubles each: [g | sum of squared errors]
    double* g;                    // P + 1: the partials added in chunk order
    const double* corr;           // (n_steps x 2) 1 - beta1^t, 1 - beta2^t of every step of this call, formed by the host
    double lr, l2;
    int n_steps;
    double *loss, *grad0, *trace; // n_steps + 1; P or nullptr; (n_steps + 1) x P or nullptr
    int* ctl;                     // [0] 0 fine, 1 the loss at the start parameters is not finite, 2 a later one; [1] steps taken
};
int launch_mlp_pack(robo_ctx* ctx, const MlpNet& net, const double* d_params, double* d_pad);
int launch_mlp_grad(robo_ctx* ctx, const MlpTrain& a, long long c0, int nc);
int launch_mlp_step(robo_ctx* ctx, const MlpTrain& a, int nc, bool first, bool final, int t);
int launch_mlp_train_one(robo_ctx* ctx, const MlpTrain& a);
int launch_mlp_forward(robo_ctx* ctx, const MlpNet& net, const double* d_rows, long long m, double* d_feat, double* d_value);

}  // namespace robo

struct robo_mlp {
    robo_ctx* ctx;
    robo::MlpNet net;             // (pad points at d_pad)
    bool has_params;
    long long steps;              // Adam steps taken since robo_mlp_set_params
    double* d_state;              // [params (P) | m (P) | v (P) | keep (3 P) | g (P + 1)]
    double* d_pad;
    int* d_ctl;
    double* d_rows;               // the uploaded rows and targets [X (n x dim) | y (n)], or the rows of a forward call (grows)
    size_t rows_cap;
    double* d_part;               // (grows)
    size_t part_cap;
    double* d_out;                // a call's [corr | loss | grad0 | trace] or [features | value] (grows)
    size_t out_cap;
};
