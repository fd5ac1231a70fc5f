// BOHAMIANN's kernels (the rule is stated in include/robo_hip.h, the owner layout in bnn_dev.h, the split of work, the LDS
// budget and the barriers in DESIGN.md).
//   bnn_chain_kernel   one workgroup per chain, many SGHMC steps per launch.  The weights are staged in LDS once and updated
//                      there in place.  A step: the mini-batch's rows are gathered by index, 16 at a time, through
//                      mlp_tile_grad (forward, deltas and dW = a^T delta on v_mfma_f64_16x16x4_f64); the gradient stays in the
//                      accumulators, and the lane that holds an entry applies that entry's sampler update: state from memory
//                      in the owner layout, the weight in LDS.  No partials, no second launch, no atomics.
//   bnn_sweep_kernel   one workgroup per 64 candidates: the rows are staged once, the S sampled networks go through
//                      mlp_features (operands from L2) one after the other, one lane per candidate folds the value and carries
//                      Welford's (mean, M2) in registers.
//   bnn_pack_kernel    the sample table -> padded layouts;  bnn_fill_kernel  the sampler's start state
#include <cmath>

#include "bnn_dev.h"
#include "philox.h"

namespace robo {

// the LDS of a chain: the gradient workgroup's (154 248 bytes) and the step's row indices, the log noise variance and two
// failure flags taken in turn (a step clears one while the last step's may still be read): 154 528 bytes of 160 KiB
struct BnnLds {
    MlpLds m;
    int idx[BNN_MAX_BATCH];
    double ell;
    int flag[2];
};

// f(q, e, p, g) for every entry this thread owns: its slot, its index in the packed [p | l], its place in LDS and what the
// gradient registers hold for it (thread 129: the sum of the squared errors)
template <class F>
__device__ __forceinline__ void bnn_for_owned(const MlpNet& s, BnnLds& b, const MlpGrad& G, F&& f) {
    const int tid = threadIdx.x, lane = tid & 63;
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        if (l < s.L) {
            const int in = mlp_in(s, l);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    int I, J;
                    if (mlp_owned_tile(s, l, i, j, I, J)) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = I * 16 + (lane >> 4) + 4 * r, col = J * 16 + (lane & 15);
                            if (row < in && col < s.H)
                                f(((l * 2 + i) * 2 + j) * 4 + r, mlp_w_off(s, l) + row * s.H + col,
                                  &b.m.W[l][row * MLP_LD + col], G.acc[l][i][j][r]);
                        }
                    }
                }
            if (tid < s.H) f(48 + l, mlp_b_off(s, l) + tid, &b.m.b[l][tid], G.gb[l]);
        }
    }
    if (tid >= 64 && tid < 64 + s.H) f(51, mlp_out_off(s) + tid - 64, &b.m.wout[tid - 64], G.side);
    else if (tid == 128) f(51, s.P - 1, &b.m.bout, G.side);
    else if (tid == 129) f(51, s.P, &b.ell, G.side);
}

// the chain's [p | l] in LDS -> dst (P + 1, packed)
__device__ __forceinline__ void bnn_store_params(const MlpNet& s, const BnnLds& b, double* __restrict__ dst) {
    const int tid = threadIdx.x, H = s.H;
    for (int l = 0; l < s.L; ++l) {
        const int in = mlp_in(s, l);
        for (int e = tid; e < in * H; e += WG) {
            const int i = e / H, j = e - i * H;
            dst[mlp_w_off(s, l) + e] = b.m.W[l][i * MLP_LD + j];
        }
        if (tid < H) dst[mlp_b_off(s, l) + tid] = b.m.b[l][tid];
    }
    if (tid < H) dst[mlp_out_off(s) + tid] = b.m.wout[tid];
    if (tid == 0) {
        dst[s.P - 1] = b.m.bout;
        dst[s.P] = b.ell;
    }
}

// one row of the trace: [p | v | tau | gbar | V], P + 1 each, of the state as it stands
__device__ __forceinline__ void bnn_trace_row(const MlpNet& s, BnnLds& b, const MlpGrad& G, const double* st, double* row) {
    const int P1 = s.P + 1;
    bnn_store_params(s, b, row);
    bnn_for_owned(s, b, G, [&](int q, int e, double*, double) {
        const double* o = st + q * WG + threadIdx.x;
#pragma unroll
        for (int a = 0; a < 4; ++a) row[(size_t)(a + 1) * P1 + e] = o[(size_t)a * BNN_OWN];
    });
}

// the sampler's update of one entry (include/robo_hip.h "Step"): mode 2 inside the burn-in, 1 M and sigma are formed from V,
// 0 they are read.  o: the entry's place in the owner layout.  -> the entry's new value.  Every operation is rounded once.
__device__ __forceinline__ double bnn_entry_step(const BnnRun& a, double* o, int mode, double p, double g, double xi) {
#pragma clang fp contract(off)
    double v = o[0], M, sig;
    if (mode != 0) {
        double V = o[(size_t)3 * BNN_OWN];
        if (mode == 2) {
            double tau = o[BNN_OWN], gbar = o[(size_t)2 * BNN_OWN];
            const double r = 1.0 / (tau + 1.0);
            tau = (tau + 1.0) - (tau * (gbar * gbar)) / V;
            gbar = gbar + r * (g - gbar);
            V = V + r * (g * g - V);
            o[BNN_OWN] = tau;
            o[(size_t)2 * BNN_OWN] = gbar;
            o[(size_t)3 * BNN_OWN] = V;
        }
        M = 1.0 / (sqrt(V) + 1e-16);
        double s2 = a.c2 * M - a.eps4;
        s2 = s2 > 1e-16 ? s2 : 1e-16;
        sig = sqrt(s2);
        o[(size_t)4 * BNN_OWN] = M;
        o[(size_t)5 * BNN_OWN] = sig;
    } else {
        M = o[(size_t)4 * BNN_OWN];
        sig = o[(size_t)5 * BNN_OWN];
    }
    v = ((v - (a.eps2 * M) * g) - a.mdecay * v) + sig * xi;
    o[0] = v;
    return p + v;
}

// the standard normal of (seed, chain, step, entry): Box-Muller's cosine branch on one Philox block
__device__ __forceinline__ double bnn_normal(unsigned long long seed, long long t, int chain, int e) {
#pragma clang fp contract(off)
    unsigned c[4] = {(unsigned)t, (unsigned)((unsigned long long)t >> 32), (unsigned)chain, (unsigned)e};
    double ua, ub;
    philox_uniform2(c, seed, ua, ub);
    const double rad = sqrt(-2.0 * log(1.0 - ua)), ang = 6.283185307179586476925 * ub;
    return rad * cos(ang);
}

__global__ __launch_bounds__(WG) void bnn_chain_kernel(BnnRun a) {
#pragma clang fp contract(off)
    __shared__ BnnLds b;
    const MlpNet& s = a.net;
    const int tid = threadIdx.x, chain = blockIdx.x, P1 = s.P + 1;
    if (a.status[2 * chain] != 0) return;                        // (the whole workgroup: the chain ended in an earlier launch)
    double* const params = a.params + (size_t)chain * P1;
    double* const st = a.state + (size_t)chain * BNN_ARRAYS * BNN_OWN;
    mlp_stage_weights(s, params, b.m);
    if (tid == 0) b.ell = params[s.P];
    __syncthreads();
    MlpGrad G;
    mlp_grad_zero(G);
    bool ended = false;
    for (int k = 0; k < a.steps; ++k) {
        const long long t = a.t0 + k, rel = t - a.call_t0;
        if (a.trace) bnn_trace_row(s, b, G, st, a.trace + ((size_t)rel * a.C + chain) * 5 * P1);
        if (tid < a.batch) {
            int i;
            if (a.idx) {
                i = a.idx[(size_t)rel * a.batch + tid];
            } else {
                unsigned c[4] = {(unsigned)t, (unsigned)((unsigned long long)t >> 32), (unsigned)chain, 0x80000000u | (unsigned)tid};
                double ua, ub;
                philox_uniform2(c, a.seed, ua, ub);
                i = (int)(ua * (double)a.n);
                if (i >= a.n) i = (int)(a.n - 1);
            }
            b.idx[tid] = i;
        }
        if (tid == 0) b.flag[k & 1] = 0;
        __syncthreads();
        const double ell = b.ell, einv = exp(-ell);
        mlp_grad_zero(G);
        for (int r0 = 0; r0 < a.batch; r0 += MLP_TR) mlp_tile_grad(s, b.m, a.rows, a.y, b.idx, r0, a.batch, einv, a.bd, G);
        // Behind mlp_tile_grad's last barrier no thread reads a weight, a bias or b.ell again in this step: the owners write.
        const int mode = t < a.burn ? 2 : (t == a.form_at ? 1 : 0);
        const double* xi = a.xi ? a.xi + ((size_t)rel * a.C + chain) * P1 : nullptr;
        bool bad = false;
        bnn_for_owned(s, b, G, [&](int q, int e, double* pp, double gd) {
            const double p = *pp;
            double g;
            if (e == s.P) g = 0.5 * (1.0 - (gd / a.bd) * einv) + (p - a.ln_mu) * a.inv_sn;
            else g = gd + a.lam_n * p;
            const double z = xi ? xi[e] : bnn_normal(a.seed, t, chain, e);
            const double pn = bnn_entry_step(a, st + q * WG + tid, mode, p, g, z);
            *pp = pn;
            bad = bad || !(fabs(pn) <= 1.79769313486231570e308);
        });
        if (bad) b.flag[k & 1] = 1;
        __syncthreads();                                          // the update is the next step's weights
        if (b.flag[k & 1] != 0) {
            if (tid == 0) {
                a.status[2 * chain] = 1;
                a.status[2 * chain + 1] = (int)rel;
            }
            ended = true;
            break;
        }
        const long long T = t + 1;
        if (T > a.burn && (T - a.burn) % a.keep == 0) {
            const long long slot = a.s0 + (bnn_keeps(T, a.burn, a.keep) - a.keeps0 - 1) * a.C + chain;
            if (slot < ROBO_BNN_MAX_SAMPLES) bnn_store_params(s, b, a.samples + (size_t)slot * P1);
        }
    }
    if (ended) return;
    bnn_store_params(s, b, params);
    if (a.final && a.trace) {
        const long long rel = a.t0 + a.steps - a.call_t0;
        bnn_trace_row(s, b, G, st, a.trace + ((size_t)rel * a.C + chain) * 5 * P1);
    }
}

// v = 0, tau = gbar = V = 1, M = sigma = 0 for every slot of every chain
__global__ __launch_bounds__(WG) void bnn_fill_kernel(double* __restrict__ state, long long total) {
    for (long long e = (long long)blockIdx.x * WG + threadIdx.x; e < total; e += (long long)gridDim.x * WG) {
        const int a = (int)((e / BNN_OWN) % BNN_ARRAYS);
        state[e] = (a >= 1 && a <= 3) ? 1.0 : 0.0;
    }
}

__global__ __launch_bounds__(WG) void bnn_pack_kernel(MlpNet s, const double* __restrict__ samples, double* __restrict__ pads) {
    const int len = mlp_pad_len(s);
    const double* p = samples + (size_t)blockIdx.y * (s.P + 1);
    double* pad = pads + (size_t)blockIdx.y * len;
    for (int e = blockIdx.x * WG + threadIdx.x; e < len; e += gridDim.x * WG) pad[e] = mlp_pad_entry(s, p, e);
}

// candidates [64 b, 64 b + 64): f_k(x) = a_L . w_out + b_out of sample k exactly as mlp_forward_kernel forms it, Welford's
// update in sample order, then the noise, the output transform and the clip.  A candidate's values depend on its row alone.
__global__ __launch_bounds__(WG) void bnn_sweep_kernel(MlpNet s, const double* __restrict__ pads,
                                                       const double* __restrict__ samples, int S,
                                                       const double* __restrict__ rows, long long m, double y_mean,
                                                       double y_std, int add_noise, double* __restrict__ out_mean,
                                                       double* __restrict__ out_var, double* __restrict__ out_ps) {
#pragma clang fp contract(off)
    constexpr int PLD = MLP_MAX + 16 + 1;
    __shared__ double sx[BLR_TC * MLP_LD];
    __shared__ double sp[BLR_TC * PLD];
    const int tid = threadIdx.x, len = mlp_pad_len(s), P1 = s.P + 1;
    const long long row0 = (long long)blockIdx.x * BLR_TC, row = row0 + tid;
    for (int e = tid; e < BLR_TC * s.DP; e += WG) {
        const int r = e / s.DP, d = e - r * s.DP;
        sx[r * MLP_LD + d] = (row0 + r < m && d < s.dim) ? rows[(size_t)(row0 + r) * s.dim + d] : 0.0;
    }
    __syncthreads();
    double mean = 0.0, M2 = 0.0, noise = 0.0;
    for (int k = 0; k < S; ++k) {
        MlpNet net = s;
        net.pad = pads + (size_t)k * len;
        mlp_features(net, row0, BLR_TC, m, sx, sp, PLD, 1, s.HP + 16);
        __syncthreads();
        if (tid < BLR_TC) {
            const double* tail = net.pad + mlp_pad_off(s, s.L);
            double f = tail[s.HP];
            for (int j = 0; j < s.H; ++j) f = fma(sp[tid * PLD + j], tail[j], f);
            const double d = f - mean;
            mean = mean + d / (double)(k + 1);
            M2 = M2 + d * (f - mean);
            if (add_noise) noise = noise + exp(samples[(size_t)k * P1 + s.P]);
            if (out_ps && row < m) out_ps[(size_t)k * m + row] = f;
        }
        __syncthreads();                                          // the next sample's features overwrite sp
    }
    if (tid < BLR_TC && row < m) {
        double var = M2 / (double)S;
        if (add_noise) var = var + noise / (double)S;
        var = var * (y_std * y_std);
        out_mean[row] = mean * y_std + y_mean;
        out_var[row] = var < BLR_EPS ? BLR_EPS : var;            // (a NaN stays a NaN)
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
int launch_bnn_fill(robo_ctx* ctx, double* d_state, int C) {
    const long long total = (long long)C * BNN_ARRAYS * BNN_OWN;
    hipLaunchKernelGGL(bnn_fill_kernel, dim3((unsigned)((total + WG - 1) / WG)), dim3(WG), 0, ctx->stream, d_state, total);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_bnn_chain(robo_ctx* ctx, const BnnRun& a) {
    hipLaunchKernelGGL(bnn_chain_kernel, dim3(a.C), dim3(WG), 0, ctx->stream, a);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_bnn_pack(robo_ctx* ctx, const MlpNet& net, const double* d_samples, int S, double* d_pads) {
    hipLaunchKernelGGL(bnn_pack_kernel, dim3((mlp_pad_len(net) + WG - 1) / WG, S), dim3(WG), 0, ctx->stream, net, d_samples, d_pads);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_bnn_sweep(robo_ctx* ctx, const MlpNet& net, const double* d_pads, const double* d_samples, int S,
                     const double* d_rows, long long m, double y_mean, double y_std, int add_noise, double* d_mean,
                     double* d_var, double* d_per_sample) {
    hipLaunchKernelGGL(bnn_sweep_kernel, dim3((unsigned)((m + BLR_TC - 1) / BLR_TC)), dim3(WG), MLP_ACT_BYTES, ctx->stream, net,
                       d_pads, d_samples, S, d_rows, m, y_mean, y_std, add_noise, d_mean, d_var, d_per_sample);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

}  // namespace robo
