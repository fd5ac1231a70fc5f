// A 128-row block's share of the log-likelihood terms: what potrf_diag_kernel (one-block likelihood), mcmc_block_step_kernel
// and mcmc_tail_kernel (the chain's fused tail) reduce -- the same operations in the same order, hence the same bits
// wherever the shares are formed.  potrf_inverse_kernel (the factorisation's tail) keeps the same operations written out.
#pragma once
#include "common.h"

namespace robo {

struct LlShare {
    double quad, logdiag;      // sum z_i^2 and sum log L_ii over the block's training rows
    double dmin, dmax;         // extreme diagonal entries of L over them (EXTREMES only)
};

// Called by all 256 threads of the workgroup's first four waves (tid = index among them); thread tid < 128 brings row tid
// of the block: valid = it is a training row, zi = its entry of z = L^-1 (y - mean), d = L_ii (both ignored when !valid).
// Wave reduction by __shfl_xor 32 .. 1, lanes 0 of waves 0 / 1 to red[0 .. 4) (red[0 .. 8) with EXTREMES), one barrier,
// then red[0] + red[1] etc. in every thread.  SYNC_FIRST: a barrier in front of the stores to red[] (callers whose red[]
// is memory the workgroup may still be reading).  The caller reads z and d from wherever they live (LDS image or global
// memory) and owns every other barrier, the one before red[] is written again included.
template <bool EXTREMES, bool SYNC_FIRST>
__device__ __forceinline__ LlShare block_ll_share(int tid, bool valid, double zi, double d, double* red) {
    double q = 0.0, lg = 0.0, dmin = __builtin_huge_val(), dmax = 0.0;
    if (valid) {
        q = zi * zi;
        lg = log(d);
        dmin = dmax = d;
    }
    for (int o = 32; o > 0; o >>= 1) {
        q += __shfl_xor(q, o);
        lg += __shfl_xor(lg, o);
        if (EXTREMES) {
            dmin = fmin(dmin, __shfl_xor(dmin, o));
            dmax = fmax(dmax, __shfl_xor(dmax, o));
        }
    }
    if (SYNC_FIRST) __syncthreads();
    if ((tid & 63) == 0 && tid < NB) {
        red[tid >> 6] = q;
        red[2 + (tid >> 6)] = lg;
        if (EXTREMES) {
            red[4 + (tid >> 6)] = dmin;
            red[6 + (tid >> 6)] = dmax;
        }
    }
    __syncthreads();
    LlShare s;
    s.quad = red[0] + red[1];
    s.logdiag = red[2] + red[3];
    s.dmin = EXTREMES ? fmin(red[4], red[5]) : 0.0;
    s.dmax = EXTREMES ? fmax(red[6], red[7]) : 0.0;
    return s;
}

}  // namespace robo
