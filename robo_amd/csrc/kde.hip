// Parzen estimators: truncated Gaussian mixtures over a box and the log-density ratio  log l(x) - log g(x)  of the
// Tree-structured Parzen Estimator (Bergstra et al. 2011), swept over candidate batches.  The density and the expansion
//     e_j(x) = c'_j + phi(x) . psi_j,   phi = [t, -t^2 / 2],  psi_j = [mu'_j / h_j^2, 1 / h_j^2]
// are stated in include/robo_hip.h.
//
//   kde_prepare_kernel   once per robo_kde_set_mixture, a component per lane: c'_j and the row psi_j, rows padded to K2 =
//                        2 D rounded up to 4, components padded to a multiple of 16 with c' = -inf, psi = 0.  No atomics.
//   kde_sweep_kernel     the hot path, both mixtures in one launch.  A workgroup (4 wave64) owns 64 candidates and forms their
//                        phi rows in LDS once; a wave owns 16 of them.  The components' psi and c' pass through LDS 64 at a
//                        time, the good mixture first.  Per 16 x 16 block a wave issues K2 / 4 v_mfma_f64_16x16x4_f64 with
//                        the COMPONENTS as the A operand (accumulator rows) and the CANDIDATES as the B operand (accumulator
//                        columns), the accumulator started at c': lane l then holds the exponents of components
//                        (l >> 4) + 4 r, r = 0 .. 3, of candidate l & 15 -- four exponents of ONE candidate, so the running
//                        log-sum-exp is lane-local: one (max, sum) pair per lane, joined with every block's part by
//                        kde_lse_join (kde_dev.h, where the -inf rule is stated).  The four lane groups of a candidate are
//                        joined at the end by two shuffles, the lower group first.  The m x n exponents are never in memory.
//
// What fixes the bits: lane group g of a candidate sums the components g + 4 r + 16 b in ascending order, the groups are
// joined (0 1) (2 3); every MFMA column depends on its own candidate alone.  So a candidate's bits depend on (its
// coordinates, the mixtures) -- not on its position in the batch, on m, on the other candidates or on the passes of the host.
//
// LDS rows have the leading dimension K2 + 2: half of it is odd, so the 16 rows of a fragment read start in 16 different
// even banks and a 32-lane half touches 32 different ones (the layout of gemm_f64.h).  The exp per pair stays on the vector
// ALU and bounds the kernel at small D; the matrix pipe takes the part proportional to D.
#include "kde_dev.h"

namespace robo {

__global__ __launch_bounds__(WG) void kde_prepare_kernel(int D, int K2, const double* __restrict__ lo,
                                                         const double* __restrict__ hi, const double* __restrict__ ctr,
                                                         const double* __restrict__ mu, const double* __restrict__ h,
                                                         int shared_h, const double* __restrict__ w, double sum_w, long long n,
                                                         int npad, double* __restrict__ psi, double* __restrict__ c) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= npad) return;
    double* row = psi + (size_t)j * K2;
    if (j >= n) {
        for (int k = 0; k < K2; ++k) row[k] = 0.0;
        c[j] = -INFINITY;
        return;
    }
    const double rs2 = 0.70710678118654752440, half_log_2pi = 0.91893853320467274178;
    double cj = log(w ? w[j] : 1.0) - log(sum_w);        // (a zero weight: -inf, and it stays -inf)
    double quad = 0.0;
    for (int d = 0; d < D; ++d) {
        const double m = mu[(size_t)j * D + d], hh = h[(shared_h ? 0 : (size_t)j * D) + d];
        // lo <= mu <= hi: the two arguments straddle 0, Z = 1 - Phi(-b) - Phi(a) with both erfc arguments >= 0
        const double a = (m - lo[d]) / hh, b = (hi[d] - m) / hh;
        const double Z = 1.0 - 0.5 * (erfc(a * rs2) + erfc(b * rs2));
        cj -= log(hh) + half_log_2pi + log(Z);
        const double ih2 = 1.0 / (hh * hh), mc = m - ctr[d];
        row[d] = mc * ih2;
        row[D + d] = ih2;
        quad += mc * mc * ih2;
    }
    for (int k = 2 * D; k < K2; ++k) row[k] = 0.0;
    c[j] = cj - 0.5 * quad;
}

template <int K2CAP>
__global__ __launch_bounds__(WG) void kde_sweep_kernel(int D, int K2, const double* __restrict__ ctr, KdeMixDev good,
                                                       KdeMixDev bad, const double* __restrict__ rows, long long m,
                                                       double* __restrict__ out_l, double* __restrict__ out_g,
                                                       double* __restrict__ out_ratio, unsigned* __restrict__ flags) {
    __shared__ double s_phi[KDE_TC * (K2CAP + 2)];
    __shared__ double s_psi[KDE_CHUNK * (K2CAP + 2)];
    __shared__ double s_c[KDE_CHUNK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, LD = K2 + 2;
    const long long row0 = (long long)blockIdx.x * KDE_TC;
    // phi rows of the tile; rows past m are 0 (their results are never written)
    for (int e = tid; e < KDE_TC * K2; e += WG) {
        const int r = e / K2, k = e - r * K2;
        double v = 0.0;
        if (row0 + r < m && k < 2 * D) {
            const int d = k < D ? k : k - D;
            const double t = rows[(size_t)(row0 + r) * D + d] - ctr[d];
            v = k < D ? t : -0.5 * t * t;
        }
        s_phi[r * LD + k] = v;
    }
    __syncthreads();
    const int col = wave * 16 + (lane & 15), grp = lane >> 4;      // this lane's candidate in the tile; its lane group
    const long long cand = row0 + col;
    const double* pb = s_phi + col * LD + grp;
    bool nan = false;
    for (int d = 0; d < D; ++d) nan = nan || s_phi[col * LD + d] != s_phi[col * LD + d];
    double logp[2] = {0.0, 0.0};
    for (int q = 0; q < 2; ++q) {
        const KdeMixDev mix = q == 0 ? good : bad;
        KdeLse run;
        run.mx = -INFINITY;
        run.sm = 0.0;
        for (int c0 = 0; c0 < mix.npad; c0 += KDE_CHUNK) {
            const int cn = mix.npad - c0 < KDE_CHUNK ? mix.npad - c0 : KDE_CHUNK;      // a multiple of 16
            __syncthreads();                                       // (the blocks of the chunk before are done)
            for (int e = tid; e < cn * K2; e += WG) {              // (contiguous in memory)
                const int r = e / K2, k = e - r * K2;
                s_psi[r * LD + k] = mix.psi[(size_t)c0 * K2 + e];
            }
            if (tid < cn) s_c[tid] = mix.c[c0 + tid];
            __syncthreads();
            for (int b0 = 0; b0 < cn; b0 += 16) {
                const double* pc = s_c + b0 + grp;
                v4d acc = {pc[0], pc[4], pc[8], pc[12]};
                const double* pa = s_psi + (b0 + (lane & 15)) * LD + grp;
                for (int k0 = 0; k0 < K2; k0 += 4) acc = mfma_f64(pa[k0], pb[k0], acc);
                run = kde_lse_join(run, kde_lse_block(acc));
            }
        }
        if (mix.npad == 0) continue;
        // the candidate's four lane groups: (0 1) (2 3), then the two halves; the lower group is the first operand
        for (int o = 16; o <= 32; o <<= 1) {
            KdeLse other;
            other.mx = __shfl_xor(run.mx, o);
            other.sm = __shfl_xor(run.sm, o);
            run = (lane & o) == 0 ? kde_lse_join(run, other) : kde_lse_join(other, run);
        }
        logp[q] = run.mx + log(run.sm);
    }
    if (grp != 0 || cand >= m) return;
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    const double ll = nan ? qnan : logp[0], lg = nan ? qnan : logp[1];
    if (good.npad != 0) out_l[cand] = ll;
    if (bad.npad != 0) out_g[cand] = lg;
    if (good.npad != 0 && bad.npad != 0) out_ratio[cand] = ll - lg;
    if (nan && flags) atomicOr(flags, (unsigned)ROBO_FLAG_NAN);
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
int launch_kde_prepare(robo_ctx* ctx, int D, const double* d_lo, const double* d_hi, const double* d_ctr, const double* d_mu,
                       const double* d_h, int shared_h, const double* d_w, double sum_w, long long n, double* d_psi, double* d_c) {
    const int npad = kde_npad(n);
    hipLaunchKernelGGL(kde_prepare_kernel, dim3((unsigned)((npad + WG - 1) / WG)), dim3(WG), 0, ctx->stream, D, kde_k2(D), d_lo,
                       d_hi, d_ctr, d_mu, d_h, shared_h, d_w, sum_w, n, npad, d_psi, d_c);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_kde_sweep(robo_ctx* ctx, int D, const double* d_ctr, const KdeMixDev& good, const KdeMixDev& bad, const double* d_rows,
                     long long m, double* d_logl, double* d_logg, double* d_ratio, unsigned* d_flags) {
    const int K2 = kde_k2(D);
    const dim3 grid((unsigned)((m + KDE_TC - 1) / KDE_TC));
    if (K2 <= KDE_K2_SMALL)
        hipLaunchKernelGGL(kde_sweep_kernel<KDE_K2_SMALL>, grid, dim3(WG), 0, ctx->stream, D, K2, d_ctr, good, bad, d_rows, m,
                           d_logl, d_logg, d_ratio, d_flags);
    else
        hipLaunchKernelGGL(kde_sweep_kernel<KDE_K2_MAX>, grid, dim3(WG), 0, ctx->stream, D, K2, d_ctr, good, bad, d_rows, m,
                           d_logl, d_logg, d_ratio, d_flags);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

}  // namespace robo
