// The hyper-parameter chain's ensemble half-step of ONE-BLOCK problems (N <= 126, the size of a Bayesian-optimisation run)
// in one launch: one workgroup per walker runs proposal, gram tiles, factorisation, likelihood and accept test.
// The launch-per-phase form of the same half-step, and the chain as a whole, are mcmc.hip; the pieces used here are the
// other kernels' own device functions (mcmc_dev.h, gram_tile.h, potrf_diag.h, loglik_dev.h).
#include "common.h"
#include "gram_tile.h"
#include "loglik_dev.h"
#include "mcmc_dev.h"
#include "potrf_diag.h"

namespace robo {

// The device-resident chain of mcmc.hip is, per half-step, proposal + scaling | gram | potrf.hip's one-block
// factorisation-with-likelihood | accept: four launches of ~5 us each around ~8 us of work at N = 40 (r03z: 34 us per
// half-step).  Here one workgroup per walker does all of it: the proposal and its metrics in LDS (mcmc_dev.h), the gram
// tiles straight into the block-packed LDS image of the diagonal block (gram_tile.h: scaling while staging, the entries
// of scale_inputs_kernel + gram_kernel bit for bit), diag128_factor_invert, potrf_diag_kernel's likelihood reductions
// (block_ll_share), the accept test (mcmc_accept_walker) and the walker's own chain record (a walker's entry for step
// `it` is final after ITS half-step).
// NG = 1: N <= 63, one 64 x 64 tile, 256 threads.  NG = 3: 64 <= N <= 126, 768 threads -- three groups of four waves
// compute the tiles (0,0), (1,0), (1,1) side by side (one after the other on four waves they took as long as the four
// launches, r03zf), then the upper two groups leave and the first one factors (a hardware barrier counts live waves).
template <int KIND, int NG>
__global__ __launch_bounds__(256 * NG) void mcmc_block_step_kernel(McmcState st, int start, int first, int h, int it,
                                                                   const double* __restrict__ X,
                                                                   const double* __restrict__ y) {
    __shared__ double smem[DIAG_SMEM_DOUBLES];
    __shared__ int sfail;
    const DiagSmem m = diag_carve(smem);
    const int grp = threadIdx.x >> 8, tid = threadIdx.x & 255, w = blockIdx.x, P = st.P, n = st.n;
    // the W image is unused until the first 16 x 16 factorisation writes its inverse: proposal and tile staging live there
    double* sq = m.sW;
    double* sism = sq + MAX_DIM + 8;
    double* sz = sism + MAX_DIM;
    int* sflag = reinterpret_cast<int*>(sz + 1);
    double* sI = sz + 2 + grp * (2 * GD * GLD + 2 * GT);     // per group: sI, sJ, sN
    double* sJ = sI + GD * GLD;
    double* sN = sJ + GD * GLD;
    static_assert(MAX_DIM + 8 + MAX_DIM + 2 + 3 * (2 * GD * GLD + 2 * GT) <= NBLK * BLK, "staging fits the W image");
    const bool ok = mcmc_block_proposal(st, start, first, h, it, w, sq, sism, sz, sflag);
    const FitSample sp = mcmc_fit_sample(st, sq, sism, ok);            // uniform, in every thread's registers
    const double z = *sz;
    double prior = 0.0;
    if (threadIdx.x == 0) {
        if (ok && st.prior_kind != 0) prior = prior_lnprob(st.prior_kind, sq, P, st.prior_par);
        if (!ok) prior = -__builtin_huge_val();
        sfail = 0;
    }
    const double q0 = tid < P ? sq[tid] : 0.0, q1 = tid + 256 < P ? sq[tid + 256] : 0.0;   // (group 0) thread p keeps q[p]
    // ---- K into the LDS image: group g owns tile (0,0) / (1,0) / (1,1); rows / columns >= n as gram_kernel writes them (gram_aug_entry)
    {
        const int bi = grp == 0 ? 0 : 1, bj = grp == 2 ? 1 : 0;
        const int tx = tid & 15, ty = tid >> 4;
        double cov[4][4];
        if (sp.direct)      // workgroup-uniform (gram_tile.h: which tile builds K for this theta)
            pair_cov_direct<KIND>(sp.cov, X, (long long)bi * GT, (long long)bj * GT, sI, sJ, cov, sism, (long long)n, tid);
        else
            pair_cov_dot<KIND>(sp.cov, X, (long long)bi * GT, (long long)bj * GT, sI, sJ, sN, cov, sism, (long long)n, tid);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int gi = bi * GT + ty * 4 + a;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int gj = bj * GT + gram_col(tx, b);
                const double val = gram_aug_entry(gi, gj, n, cov[a][b], sp.noise, y, sp.mean_c);
                if ((gj >> 4) <= (gi >> 4)) m.sL[blk_off(gi >> 4, gj >> 4) + bidx(gi & 15, gj & 15)] = val;
            }
        }
    }
    __syncthreads();
    if (grp != 0) return;
    // (diag128_factor_invert stops after the sub-blocks that hold rows <= n: the blocks behind them are never read)
    diag128_factor_invert(m.sL, m.sW, m.sT, m.sRd, m.sCol, 0, n, &sfail, nullptr);
    // ---- (z.z, 2 sum log L_ii): the operations of potrf_diag_kernel's one-block branch, in its order
    __syncthreads();
    const bool valid = tid < NB && tid < n;
    double zi = 0.0, d = 0.0;
    if (valid) {
        zi = m.sL[blk_off(n >> 4, tid >> 4) + bidx(n & 15, tid & 15)];
        d = m.sL[blk_off(tid >> 4, tid >> 4) + bidx(tid & 15, tid & 15)];
    }
    const LlShare s = block_ll_share<false, true>(tid, valid, zi, d, m.sW);
    // ---- accept test (mcmc_accept_kernel's, for this walker)
    const int half = st.k / 2, sw = start ? first + w : h * half + w;
    if (tid == 0) *sflag = mcmc_accept_walker(st, start, h, it, w, sw, prior, sfail, false, s.quad, 2.0 * s.logdiag, &z);
    __syncthreads();
    if (start) return;
    const bool acc = *sflag != 0;
    for (int p = tid, e = 0; p < P; p += 256, ++e) {
        double* pp = st.d_pos + (size_t)sw * P + p;
        const double v = acc ? (e == 0 ? q0 : q1) : *pp;
        if (acc) *pp = v;
        if (st.d_chain) st.d_chain[((size_t)sw * st.n_steps + it) * P + p] = v;
    }
}

int launch_mcmc_block_step(robo_gp* gp, const McmcState& st, int start, int first, int h, int it) {
    const int ns = start ? st.ns_eval : st.k / 2;
    const bool one_tile = gp->n + 1 <= GT;
#define ROBO_BLOCK_STEP(KIND, NG)                                                                                     \
    hipLaunchKernelGGL((mcmc_block_step_kernel<KIND, NG>), dim3(ns), dim3(256 * NG), 0, gp->ctx->stream, st, start, first, \
                       h, it, (const double*)gp->d_X, (const double*)gp->d_y)
    if (gp->kind == ROBO_KERNEL_MATERN52_ARD) {
        if (one_tile) ROBO_BLOCK_STEP(ROBO_KERNEL_MATERN52_ARD, 1);
        else ROBO_BLOCK_STEP(ROBO_KERNEL_MATERN52_ARD, 3);
    } else {
        if (one_tile) ROBO_BLOCK_STEP(ROBO_KERNEL_RBF_ARD, 1);
        else ROBO_BLOCK_STEP(ROBO_KERNEL_RBF_ARD, 3);
    }
#undef ROBO_BLOCK_STEP
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

}  // namespace robo
