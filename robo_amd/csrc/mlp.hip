// A small tanh network trained by full-batch Adam: the kernels (the rule is stated in include/robo_hip.h, the layouts in
// mlp_dev.h, the split of work and the LDS budget in DESIGN.md).
//   mlp_grad_kernel       one workgroup per chunk of BLR_CHUNK rows.  All layers' weights are staged in LDS once; the rows go
//                         through in tiles of 16.  Forward: layer by layer on v_mfma_f64_16x16x4_f64, wave w the w-th 16
//                         units, every layer's activations kept in LDS.  Backward: delta_L on the vector pipe, then per layer
//                         dW_l += a_(l-1)^T delta_l (the four waves own the quadrants of dW_l's tile grid, accumulators in
//                         registers across the chunk's tiles) and delta_(l-1) = (delta_l W_l^T) (1 - a_(l-1)^2), both on the
//                         matrix pipe.  Bias gradients, the output layer and the loss ride along on the vector pipe, every
//                         sum in row order.  One partial [g (P) | sum of squared errors] per chunk.
//   mlp_step_kernel       ONE workgroup: the partials added in chunk order, the l2 terms, the loss, Adam.  No atomics anywhere.
//   mlp_train_one_kernel  n <= BLR_CHUNK: the whole loop in one launch by one workgroup that calls the two device functions
//                         above step after step -- the per-step form's bits.
//   mlp_pack_kernel       packed -> padded parameters;  mlp_forward_kernel  64 rows per workgroup through mlp_features
#include <cmath>

#include "blr_dev.h"

namespace robo {

// rows [beg, end) -> out[0 .. P - 1] = d (sum of squared errors / n) / d p, out[P] = the sum of squared errors.  The weights
// are in LDS (mlp_stage_weights); the tiles go through mlp_tile_grad (mlp_dev.h).  Every thread of the workgroup calls it;
// ends on a barrier.
__device__ __forceinline__ void mlp_chunk_grad(const MlpNet& s, MlpLds& m, const double* __restrict__ rows,
                                               const double* __restrict__ y, double n, long long beg, long long end,
                                               double* out) {
    const int tid = threadIdx.x, lane = tid & 63, H = s.H;
    const int tiles = (int)((end - beg + MLP_TR - 1) / MLP_TR);
    MlpGrad G;
    mlp_grad_zero(G);
    for (int t = 0; t < tiles; ++t) mlp_tile_grad(s, m, rows, y, nullptr, beg + (long long)t * MLP_TR, end, 2.0, n, G);
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        if (l < s.L) {
            const int in = mlp_in(s, l);
            double* gW = out + mlp_w_off(s, l);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    int I, J;
                    if (mlp_owned_tile(s, l, i, j, I, J)) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = I * 16 + (lane >> 4) + 4 * r, col = J * 16 + (lane & 15);
                            if (row < in && col < H) gW[row * H + col] = G.acc[l][i][j][r];
                        }
                    }
                }
            if (tid < H) out[mlp_b_off(s, l) + tid] = G.gb[l];
        }
    }
    if (tid >= 64 && tid < 64 + H) out[mlp_out_off(s) + tid - 64] = G.side;
    else if (tid == 128) out[s.P - 1] = G.side;
    else if (tid == 129) out[s.P] = G.side;
    __syncthreads();
}

// g (+)= the nc partials in chunk order; with `final`, step t of the call: the loss at the current parameters, the l2 terms,
// the records the call asked for and -- unless t is the evaluation behind the last step -- Adam's update.  A loss that is not
// finite ends the run: at t = 0 nothing has moved, later the parameters and moments of the step before are put back.  Every
// operation is rounded once (nothing contracted): the two kernels that call it then make the same bits.
__device__ __forceinline__ void mlp_step(const MlpTrain& a, int nc, bool first, bool final, int t, double* red) {
#pragma clang fp contract(off)
    const MlpNet& s = a.net;
    const int tid = threadIdx.x, P = s.P;
    const int status = a.ctl[0];
    __syncthreads();
    if (status != 0) return;
    for (int e = tid; e <= P; e += WG) {
        double sum = first ? 0.0 : a.g[e];
        for (int c = 0; c < nc; ++c) sum = sum + a.part[(size_t)c * (P + 1) + e];
        a.g[e] = sum;
    }
    if (!final) return;
    double w2 = 0.0;
    for (int e = tid; e < P; e += WG)
        if (mlp_is_weight(s, e)) w2 = fma(a.params[e], a.params[e], w2);
    red[tid] = w2;
    __syncthreads();                                              // (g[P] is another thread's store: also behind this barrier)
    if (tid == 0) {
        double sum = 0.0;
        for (int i = 0; i < WG; ++i) sum = sum + red[i];
        red[0] = a.g[P] / (double)a.n + a.l2 * sum;
    }
    __syncthreads();
    const double loss = red[0];
    __syncthreads();
    double* const m = a.mom;
    double* const v = a.mom + P;
    if (!(fabs(loss) <= 1.79769313486231570e308)) {
        if (t > 0)
            for (int e = tid; e < P; e += WG) {
                a.params[e] = a.keep[e];
                m[e] = a.keep[P + e];
                v[e] = a.keep[2 * P + e];
            }
        if (tid == 0) {
            a.ctl[0] = t == 0 ? 1 : 2;
            a.ctl[1] = t > 0 ? t - 1 : 0;
        }
        return;
    }
    if (tid == 0) {
        a.loss[t] = loss;
        a.ctl[1] = t;
    }
    const bool update = t < a.n_steps;
    const double c1 = update ? a.corr[2 * t] : 1.0, c2 = update ? a.corr[2 * t + 1] : 1.0;
    for (int e = tid; e < P; e += WG) {
        const double p = a.params[e];
        const double g = mlp_is_weight(s, e) ? a.g[e] + (2.0 * a.l2) * p : a.g[e];
        if (a.trace) a.trace[(size_t)t * P + e] = p;
        if (t == 0 && a.grad0) a.grad0[e] = g;
        if (!update) continue;
        a.keep[e] = p;
        a.keep[P + e] = m[e];
        a.keep[2 * P + e] = v[e];
        const double mn = 0.9 * m[e] + (1.0 - 0.9) * g;
        const double vn = 0.999 * v[e] + (1.0 - 0.999) * (g * g);
        m[e] = mn;
        v[e] = vn;
        a.params[e] = p - (a.lr * (mn / c1)) / (sqrt(vn / c2) + 1e-8);
    }
}

__global__ __launch_bounds__(WG) void mlp_grad_kernel(MlpTrain a, long long c0) {
    __shared__ MlpLds m;
    mlp_stage_weights(a.net, a.params, m);
    const long long beg = (c0 + blockIdx.x) * BLR_CHUNK;
    const long long end = beg + BLR_CHUNK < a.n ? beg + BLR_CHUNK : a.n;
    mlp_chunk_grad(a.net, m, a.rows, a.y, (double)a.n, beg, end, a.part + (size_t)blockIdx.x * (a.net.P + 1));
}

__global__ __launch_bounds__(WG) void mlp_step_kernel(MlpTrain a, int nc, int first, int final, int t) {
    __shared__ double red[WG];
    mlp_step(a, nc, first != 0, final != 0, t, red);
}

__global__ __launch_bounds__(WG) void mlp_train_one_kernel(MlpTrain a) {
    __shared__ MlpLds m;
    for (int t = 0; t <= a.n_steps; ++t) {
        mlp_stage_weights(a.net, a.params, m);
        mlp_chunk_grad(a.net, m, a.rows, a.y, (double)a.n, 0, a.n, a.part);
        mlp_step(a, 1, true, true, t, m.red);
        __syncthreads();                                          // (the update's stores are this workgroup's own next reads)
        if (a.ctl[0] != 0) break;
    }
}

__global__ __launch_bounds__(WG) void mlp_pack_kernel(MlpNet s, const double* __restrict__ p, double* __restrict__ pad) {
    const int len = mlp_pad_len(s);
    for (int e = blockIdx.x * WG + threadIdx.x; e < len; e += gridDim.x * WG) pad[e] = mlp_pad_entry(s, p, e);
}

// rows [64 b, 64 b + 64): the features [a_L, 1] (nullable) and the value a_L . w_out + b_out (nullable), units in index order
__global__ __launch_bounds__(WG) void mlp_forward_kernel(MlpNet s, const double* __restrict__ rows, long long m,
                                                         double* __restrict__ feat, double* __restrict__ value) {
    constexpr int PLD = MLP_MAX + 16 + 1;
    __shared__ double sx[BLR_TC * MLP_LD];
    __shared__ double sp[BLR_TC * PLD];
    const long long row0 = (long long)blockIdx.x * BLR_TC;
    const int F = s.H + 1;
    for (int e = threadIdx.x; e < BLR_TC * s.DP; e += WG) {
        const int r = e / s.DP, d = e - r * s.DP;
        sx[r * MLP_LD + d] = (row0 + r < m && d < s.dim) ? rows[(size_t)(row0 + r) * s.dim + d] : 0.0;
    }
    __syncthreads();
    mlp_features(s, row0, BLR_TC, m, sx, sp, PLD, 1, s.HP + 16);
    __syncthreads();
    if (feat)
        for (int e = threadIdx.x; e < BLR_TC * F; e += WG) {
            const int r = e / F, f = e - r * F;
            if (row0 + r < m) feat[(size_t)(row0 + r) * F + f] = sp[r * PLD + f];
        }
    if (value && threadIdx.x < BLR_TC && row0 + threadIdx.x < m) {
        const double* tail = s.pad + mlp_pad_off(s, s.L);
        double f = tail[s.HP];
        for (int j = 0; j < s.H; ++j) f = fma(sp[threadIdx.x * PLD + j], tail[j], f);
        value[row0 + threadIdx.x] = f;
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
int launch_mlp_pack(robo_ctx* ctx, const MlpNet& net, const double* d_params, double* d_pad) {
    hipLaunchKernelGGL(mlp_pack_kernel, dim3((mlp_pad_len(net) + WG - 1) / WG), dim3(WG), 0, ctx->stream, net, d_params, d_pad);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_mlp_grad(robo_ctx* ctx, const MlpTrain& a, long long c0, int nc) {
    hipLaunchKernelGGL(mlp_grad_kernel, dim3(nc), dim3(WG), 0, ctx->stream, a, c0);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_mlp_step(robo_ctx* ctx, const MlpTrain& a, int nc, bool first, bool final, int t) {
    hipLaunchKernelGGL(mlp_step_kernel, dim3(1), dim3(WG), 0, ctx->stream, a, nc, first ? 1 : 0, final ? 1 : 0, t);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_mlp_train_one(robo_ctx* ctx, const MlpTrain& a) {
    hipLaunchKernelGGL(mlp_train_one_kernel, dim3(1), dim3(WG), 0, ctx->stream, a);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_mlp_forward(robo_ctx* ctx, const MlpNet& net, const double* d_rows, long long m, double* d_feat, double* d_value) {
    hipLaunchKernelGGL(mlp_forward_kernel, dim3((unsigned)((m + BLR_TC - 1) / BLR_TC)), dim3(WG), MLP_ACT_BYTES, ctx->stream, net,
                       d_rows, m, d_feat, d_value);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

}  // namespace robo
