// CMA-ES over a closed-form acquisition, resident on the device: the kernels (robo_acq_cmaes_cand,
// robo_acq_cmaes_marginal_cand; the rule is stated in include/robo_hip.h, the driver is api_cmaes.hip).
//
// The reference's CMAES maximiser (robo/maximizers/cmaes.py) drives the `cma` package from the host, one 1 x D acquisition
// call per function value.  Here R independent instances of Hansen's (mu/mu_w, lambda)-CMA-ES advance in lock step, one
// workgroup of 256 lanes per instance, with launches only:
//
//   cma_init_kernel     instance r := the r-th best candidate of the sweep (refine.hip's selection), C = A = A^-1 = I
//   cma_ask_kernel      A and the lambda draws z_i (the caller's, or Philox + Box-Muller) into LDS, Y = Z A on
//                       v_mfma_f64_16x16x4_f64, x_i = clip(m + sigma y_i, 0, 1), y_i := (x_i - m) / sigma, the points scaled
//                       by every model's metrics into that model's candidate handle
//   (per model)         the posterior of the R lambda points: predict_scaled, as robo_acq_eval runs it for such a batch
//   cma_tell_kernel     acquisition values from the resident moments (mean over the models in order), ranking by counting,
//                       y_w, m, p_sigma (through A^-1), h_sigma, p_c, sigma on the vector ALU; the covariance update
//                       a C + c_1 p_c p_c^T + (c_mu Y_sel diag(w)) Y_sel^T on the matrix instruction, upper tile triangle
//                       mirrored; when due the eigendecomposition of C by cyclic two-sided Jacobi in LDS (round-robin
//                       pairs, every round's disjoint rotations applied to the whole matrix at once) and
//                       A = (B sqrt(Lambda)) B^T, A^-1 = (B / sqrt(Lambda)) B^T on the matrix instruction again
//   cma_result_kernel   the best-so-far of the best instance
//
// Every matrix lives in LDS as [CMA_MAX][CMA_LD] with D and lambda padded to multiples of 16 by ZEROS, so pad rows and
// columns contribute exact zeros to every product.  LDS: the ask kernel holds three such matrices (A, Z, Y: 99 KB), the
// tell kernel four (C / Jacobi ping, Jacobi pong / c_mu w y, Y_sel / B diag, A^-1 / B: 132 KB + 5 KB of vectors) of the
// 160 KB of a gfx950 CU: one workgroup per CU, and R <= 64 of 256 CUs are busy.  An instance never looks at another one.
#include "kern_math.h"
#include "philox.h"

namespace robo {

constexpr int CMA_MAT = CMA_MAX * CMA_LD;
constexpr int CMA_EIG_MAX_SWEEPS = 40;
constexpr double CMA_EPS = 2.220446049250313e-16;
constexpr double CMA_EIG_THRESHOLD = 2.0 * CMA_EPS;      // |g_pq| <= this * max(sqrt(|g_pp g_qq|), eps trace): rotated away
constexpr double CMA_COND_MAX = 1e14;
constexpr double CMA_DBL_MAX = 1.79769313486231570e308;

__device__ __forceinline__ bool cma_finite(double v) { return fabs(v) <= CMA_DBL_MAX; }
__device__ __forceinline__ int cma_pad16(int n) { return (n + 15) / 16 * 16; }

// Out[i][j] = init(i, j) + sum_{k < kp} P[i][k] Q[j][k] over the 16 x 16 tiles (ti < nti, tj < ntj; upper: ti <= tj only),
// tile t on wave t mod 4; P, Q in LDS with leading dimension CMA_LD, kp a multiple of 4.  Fragment maps: gemm_f64.h.
template <class Init, class Store>
__device__ __forceinline__ void cma_mm_nt(const double* P, const double* Q, int nti, int ntj, int kp, bool upper, Init init,
                                          Store store) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = wave; t < nti * ntj; t += 4) {
        const int ti = t / ntj, tj = t - ti * ntj;
        if (upper && ti > tj) continue;
        const int row0 = ti * 16 + (lane >> 4), col = tj * 16 + (lane & 15);
        v4d acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = init(row0 + 4 * r, col);
        const double* pa = P + (ti * 16 + (lane & 15)) * CMA_LD + (lane >> 4);
        const double* pb = Q + (tj * 16 + (lane & 15)) * CMA_LD + (lane >> 4);
        for (int k0 = 0; k0 < kp; k0 += 4) acc = mfma_f64(pa[k0], pb[k0], acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) store(row0 + 4 * r, col, acc[r]);
    }
}

// the state columns of a trace row (m, sigma, p_sigma, p_c, h_sigma, code, C, A, A^-1) from the instance's arrays
__device__ __forceinline__ void cma_trace_state(const CmaState& st, int r, double* row, double hs, int code) {
    const int D = st.D, L = st.L, tid = threadIdx.x, nt = blockDim.x;
    double* p = row + (size_t)3 * L * D + 2 * L;
    for (int d = tid; d < D; d += nt) {
        p[d] = st.m[(size_t)r * D + d];
        p[D + 1 + d] = st.ps[(size_t)r * D + d];
        p[2 * D + 1 + d] = st.pc[(size_t)r * D + d];
    }
    if (tid == 0) {
        p[D] = st.sigma[r];
        p[3 * D + 1] = hs;
        p[3 * D + 2] = (double)code;
    }
    double* q = p + 3 * D + 3;
    const size_t dd = (size_t)D * D;
    for (size_t e = tid; e < dd; e += nt) {
        q[e] = st.C[r * dd + e];
        q[dd + e] = st.A[r * dd + e];
        q[2 * dd + e] = st.Ainv[r * dd + e];
    }
}

// one workgroup per instance: the r-th selected candidate (refine.hip's gather has put point and sweep value into `sel`)
__global__ __launch_bounds__(64) void cma_init_kernel(CmaState st, RefineState sel) {
    const int r = blockIdx.x, D = st.D, L = st.L, tid = threadIdx.x;
    const bool used = sel.start[r] >= 0;
    for (int d = tid; d < D; d += 64) {
        const double v = used ? sel.x[(size_t)r * D + d] : 0.0;
        st.m[(size_t)r * D + d] = v;
        st.bestx[(size_t)r * D + d] = v;
        st.ps[(size_t)r * D + d] = 0.0;
        st.pc[(size_t)r * D + d] = 0.0;
    }
    const size_t dd = (size_t)D * D;
    for (size_t e = tid; e < dd; e += 64) {
        const double v = e / D == e % D ? 1.0 : 0.0;
        st.C[r * dd + e] = v;
        st.A[r * dd + e] = v;
        st.Ainv[r * dd + e] = v;
    }
    if (tid == 0) {
        st.sigma[r] = st.sigma0;
        st.bestf[r] = used ? sel.f[r] : -__builtin_huge_val();
        st.gen[r] = 0;
        st.frozen[r] = used ? CMA_LIVE : CMA_UNUSED;
        if (r == 0) *st.flags = 0u;
    }
    if (!st.trace) return;
    __syncthreads();
    double* row = st.trace + (size_t)r * cma_trace_row(D, L);
    for (int e = tid; e < 3 * L * D + 2 * L; e += 64) row[e] = 0.0;
    cma_trace_state(st, r, row, 0.0, used ? CMA_LIVE : CMA_UNUSED);
}

__global__ __launch_bounds__(WG) void cma_ask_kernel(CmaState st, int g) {
    __shared__ double sA[CMA_MAT], sZ[CMA_MAT], sY[CMA_MAT];
    const int r = blockIdx.x, tid = threadIdx.x, D = st.D, L = st.L, S = st.S;
    const int DP = cma_pad16(D), LP = cma_pad16(L);
    const bool live = st.frozen[r] == CMA_LIVE;
    double* row = st.trace ? st.trace + ((size_t)(g + 1) * st.R + r) * cma_trace_row(D, L) : nullptr;
    if (live) {
        for (int e = tid; e < CMA_MAT; e += WG) {
            sA[e] = 0.0;
            sZ[e] = 0.0;
        }
        __syncthreads();
        const double* A = st.A + (size_t)r * D * D;
        for (int e = tid; e < D * D; e += WG) sA[(e / D) * CMA_LD + e % D] = A[e];
        if (st.z) {
            const double* z = st.z + ((size_t)g * st.R + r) * L * D;
            for (int e = tid; e < L * D; e += WG) sZ[(e / D) * CMA_LD + e % D] = z[e];
        } else {
            // the pair (2 p, 2 p + 1) of sample i: both Box-Muller branches of the Philox block (g, r, i, p)
            const int np = (D + 1) / 2;
            for (int e = tid; e < L * np; e += WG) {
                const int i = e / np, p = e - i * np;
                unsigned c[4] = {(unsigned)g, (unsigned)r, (unsigned)i, (unsigned)p};
                double ua, ub;
                philox_uniform2(c, st.seed, ua, ub);
                const double rad = sqrt(-2.0 * log(1.0 - ua)), ang = 6.283185307179586476925 * ub;
                sZ[i * CMA_LD + 2 * p] = rad * cos(ang);
                if (2 * p + 1 < D) sZ[i * CMA_LD + 2 * p + 1] = rad * sin(ang);
            }
        }
        __syncthreads();
        // Y[i][d] = sum_k Z[i][k] A[d][k]  (A is symmetric)
        cma_mm_nt(sZ, sA, LP / 16, DP / 16, DP, false, [](int, int) { return 0.0; },
                  [&](int i, int d, double v) { sY[i * CMA_LD + d] = v; });
        __syncthreads();
    }
    const double sigma = st.sigma[r];
    for (int e = tid; e < L * D; e += WG) {
        const int i = e / D, d = e - i * D;
        const size_t at = ((size_t)r * L + i) * D + d;
        double x, z = 0.0, y = 0.0;
        if (live) {
            const double m = st.m[(size_t)r * D + d];
            z = sZ[i * CMA_LD + d];
            x = m + sigma * sY[i * CMA_LD + d];
            x = x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x);        // (a NaN stays: the tell kernel ranks its value last)
            y = (x - m) / sigma;
            st.x[at] = x;
            st.y[at] = y;
        } else {
            x = st.bestx[(size_t)r * D + d];                 // a stopped instance hands finite rows to the solve
        }
        for (int s = 0; s < S; ++s) st.model[s].Xcs[at] = x * st.model[s].ism[d];
        if (row) {
            row[e] = z;
            row[L * D + e] = live ? x : 0.0;
            row[2 * L * D + e] = y;
        }
    }
    if (r != 0) return;
    // rows of the handles beyond R lambda replicate row 0, as scale_inputs_kernel's pad rows do
    __syncthreads();
    const long long first = (long long)st.R * L * D, last = st.m_pad * D;
    for (int s = 0; s < S; ++s) {
        double* X = st.model[s].Xcs;
        for (long long e = first + tid; e < last; e += WG) X[e] = X[e % D];
    }
}

__global__ __launch_bounds__(WG) void cma_tell_kernel(CmaState st, int g) {
    __shared__ double sC[CMA_MAT], sP[CMA_MAT], sQ[CMA_MAT], sB[CMA_MAT];
    __shared__ double s_val[CMA_MAX], s_yw[CMA_MAX], s_ps[CMA_MAX], s_pc[CMA_MAX];
    __shared__ double s_al[CMA_MAX], s_be[CMA_MAX], s_cs[CMA_MAX / 2][2], s_red[CMA_MAX / 2];
    __shared__ int s_rank[CMA_MAX], s_ord[CMA_MAX], s_part[CMA_MAX], s_pq[CMA_MAX / 2][2];
    __shared__ double s_hs, s_floor;
    __shared__ int s_nfin, s_code;
    const int r = blockIdx.x, tid = threadIdx.x, D = st.D, L = st.L, S = st.S, mu = st.mu;
    const int DP = cma_pad16(D);
    const size_t dd = (size_t)D * D;
    double* row = st.trace ? st.trace + ((size_t)(g + 1) * st.R + r) * cma_trace_row(D, L) : nullptr;
    double* tval = row ? row + (size_t)3 * L * D : nullptr;
    const int code0 = st.frozen[r];
    if (code0 != CMA_LIVE) {
        if (row) {
            for (int e = tid; e < 2 * L; e += WG) tval[e] = 0.0;
            cma_trace_state(st, r, row, 0.0, code0 == CMA_UNUSED ? CMA_UNUSED : CMA_WAS_FROZEN);
        }
        return;
    }
    const double sigma = st.sigma[r], bestf = st.bestf[r];
    for (int e = tid; e < CMA_MAT; e += WG) {
        sC[e] = 0.0;
        sP[e] = 0.0;
        sQ[e] = 0.0;
        sB[e] = 0.0;
    }
    if (tid < CMA_MAX) s_pc[tid] = 0.0;
    // ---- acquisition values: the mean over the models in order (refine.hip's rule), guards as acq_kernel's
    if (tid < L) {
        const size_t at = (size_t)r * L + tid;
        double facc = 0.0;
        unsigned f = 0;
        for (int s = 0; s < S; ++s) {
            const CmaModel md = st.model[s];
            const double mean = md.mean[at], v = md.var[at];
            double lp;
            if (st.kind == ROBO_ACQ_EI) {
                lp = acq_ei(mean, v, md.eta, st.par);
                if (lp < 0.0 && lp > -2.2250738585072014e-308) lp = 0.0;
                if (lp < 0.0) f |= ROBO_FLAG_NEGATIVE_EI;
            } else if (st.kind == ROBO_ACQ_LOG_EI) {
                lp = acq_log_ei(mean, v, md.eta, st.par);
            } else if (st.kind == ROBO_ACQ_PI) {
                lp = acq_pi(mean, v, md.eta, st.par);
            } else {
                lp = acq_lcb(mean, v, st.par);
            }
            if (sqrt(v) == 0.0) f |= ROBO_FLAG_ZERO_SIGMA;
            facc = s > 0 ? facc + lp : lp;
        }
        const double val = rn_div(facc, (double)S);
        if (val != val) f |= ROBO_FLAG_NAN;
        if (f != 0) atomicOr(st.flags, f);
        s_val[tid] = val;
    }
    __syncthreads();
    // ---- ranking by counting: descending value, ties by ascending index, NaN last
    if (tid < L) {
        const double vi = s_val[tid];
        const bool ni = vi != vi;
        int rank = 0;
        for (int j = 0; j < L; ++j) {
            const double vj = s_val[j];
            const bool nj = vj != vj;
            const bool better = ni ? (!nj || j < tid) : (!nj && (vj > vi || (vj == vi && j < tid)));
            rank += better ? 1 : 0;
        }
        s_rank[tid] = rank;
        s_ord[rank] = tid;
    }
    if (tid == 0) {
        int n = 0;
        for (int j = 0; j < L; ++j) n += cma_finite(s_val[j]) ? 1 : 0;
        s_nfin = n;
        s_code = CMA_LIVE;
    }
    __syncthreads();
    if (row)
        for (int e = tid; e < L; e += WG) {
            tval[e] = s_val[e];
            tval[L + e] = (double)s_rank[e];
        }
    if (s_nfin == 0) {                   // nothing to rank by: the instance stops where it is
        if (tid == 0) {
            st.frozen[r] = CMA_ALL_BAD;
            atomicOr(st.flags, ROBO_FLAG_FROZEN);
        }
        if (row) cma_trace_state(st, r, row, 0.0, CMA_ALL_BAD);
        return;
    }
    // ---- best-so-far: replaced only by a strictly larger value
    {
        const int i0 = s_ord[0];
        if (s_val[i0] > bestf) {
            if (tid < D) st.bestx[(size_t)r * D + tid] = st.x[((size_t)r * L + i0) * D + tid];
            if (tid == 0) st.bestf[r] = s_val[i0];
        }
    }
    // ---- staging: Y_sel and c_mu w Y_sel as [d][k], A^-1, C
    for (int e = tid; e < mu * D; e += WG) {
        const int k = e / D, d = e - k * D;
        const double y = st.y[((size_t)r * L + s_ord[k]) * D + d];
        sQ[d * CMA_LD + k] = y;
        sP[d * CMA_LD + k] = st.cmu * st.w[k] * y;
    }
    for (int e = tid; e < D * D; e += WG) {
        sB[(e / D) * CMA_LD + e % D] = st.Ainv[r * dd + e];
        sC[(e / D) * CMA_LD + e % D] = st.C[r * dd + e];
    }
    __syncthreads();
    if (tid < D) {
        double yw = 0.0;
        for (int k = 0; k < mu; ++k) yw += st.w[k] * sQ[tid * CMA_LD + k];
        s_yw[tid] = yw;
        // a convex combination of points of the box: it can leave the box by a rounding only, and is put back
        const double mn = st.m[(size_t)r * D + tid] + sigma * yw;
        st.m[(size_t)r * D + tid] = mn < 0.0 ? 0.0 : (mn > 1.0 ? 1.0 : mn);
    }
    __syncthreads();
    if (tid < D) {
        double v = 0.0;
        for (int e = 0; e < D; ++e) v += sB[tid * CMA_LD + e] * s_yw[e];
        const double ps = (1.0 - st.cs) * st.ps[(size_t)r * D + tid] + sqrt(st.cs * (2.0 - st.cs) * st.mueff) * v;
        s_ps[tid] = ps;
        st.ps[(size_t)r * D + tid] = ps;
    }
    __syncthreads();
    if (tid == 0) {
        double n2 = 0.0;
        for (int d = 0; d < D; ++d) n2 += s_ps[d] * s_ps[d];
        const double pn = sqrt(n2);
        const double den = sqrt(1.0 - exp(2.0 * (double)(g + 1) * st.log1mcs));
        s_hs = pn / den < (1.4 + 2.0 / ((double)D + 1.0)) * st.chin ? 1.0 : 0.0;
        const double sn = sigma * exp(st.cs / st.ds * (pn / st.chin - 1.0));
        st.sigma[r] = sn;
        if (!cma_finite(sn)) s_code = CMA_SIGMA_BAD;
        else if (sn < st.sigma_min) s_code = CMA_SIGMA_MIN;
    }
    __syncthreads();
    const double hs = s_hs;
    const int code_sigma = s_code;       // read behind the barrier that follows the step-size update: uniform, and no later
                                         // store to s_code can reach a wave that has not decided `due` yet
    if (tid < D) {
        const double pc = (1.0 - st.cc) * st.pc[(size_t)r * D + tid] + hs * sqrt(st.cc * (2.0 - st.cc) * st.mueff) * s_yw[tid];
        s_pc[tid] = pc;
        st.pc[(size_t)r * D + tid] = pc;
    }
    __syncthreads();
    // ---- C <- a C + c_1 p_c p_c^T + (c_mu Y_sel diag(w)) Y_sel^T: upper tile triangle on the matrix instruction, mirrored
    {
        const double a = (1.0 - st.c1 - st.cmu) + st.c1 * (1.0 - hs) * st.cc * (2.0 - st.cc), c1 = st.c1;
        cma_mm_nt(sP, sQ, DP / 16, DP / 16, (mu + 3) / 4 * 4, true,
                  [&](int i, int j) { return i <= j ? a * sC[i * CMA_LD + j] + c1 * s_pc[i] * s_pc[j] : 0.0; },
                  [&](int i, int j, double v) {
                      if (i <= j && j < D) {
                          sC[i * CMA_LD + j] = v;
                          sC[j * CMA_LD + i] = v;
                      }
                  });
    }
    __syncthreads();
    for (int e = tid; e < D * D; e += WG) st.C[r * dd + e] = sC[(e / D) * CMA_LD + e % D];
    // ---- when due: C = B Lambda B^T by cyclic two-sided Jacobi, G ping-ponging between sC and sP, B in sB
    const bool due = code_sigma == CMA_LIVE && (g + 1) % st.eig_every == 0;
    if (due) {
        double *G = sC, *H = sP;
        for (int e = tid; e < CMA_MAT; e += WG) sB[e] = (e / CMA_LD == e % CMA_LD && e / CMA_LD < D) ? 1.0 : 0.0;
        if (tid == 0) {
            double tr = 0.0;
            for (int i = 0; i < D; ++i) tr += fabs(G[i * CMA_LD + i]);
            s_floor = tr * CMA_EPS;
            if (!cma_finite(tr)) s_code = CMA_EIG_BAD;
        }
        __syncthreads();
        const int M = (D + 1) / 2 * 2, np = M / 2, rounds = M - 1;
        bool converged = s_code != CMA_LIVE;
        for (int sweep = 0; sweep < CMA_EIG_MAX_SWEEPS && !converged; ++sweep) {
            double off = 0.0;
            for (int rd = 0; rd < rounds; ++rd) {
                if (tid < np) {          // the circle method's pair of this lane; a pair with player D (odd D) is idle
                    const int u = (rd + tid) % (M - 1), w = tid == 0 ? M - 1 : (rd - tid + (M - 1)) % (M - 1);
                    const int p = u < w ? u : w, q = u < w ? w : u;
                    double c = 1.0, s = 0.0;
                    if (q < D) {
                        const double gpp = G[p * CMA_LD + p], gqq = G[q * CMA_LD + q], gpq = G[p * CMA_LD + q];
                        if (gpq != 0.0) {
                            const double ratio = fabs(gpq) / fmax(sqrt(fabs(gpp * gqq)), s_floor);
                            off = fmax(off, ratio);
                            if (!(ratio <= CMA_EIG_THRESHOLD)) {
                                const double tau = (gqq - gpp) / (2.0 * gpq);
                                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                                c = 1.0 / sqrt(1.0 + t * t);
                                s = t * c;
                            }
                        }
                        s_part[q] = p;
                        s_al[q] = c;
                        s_be[q] = s;
                    }
                    s_part[p] = q < D ? q : p;
                    s_al[p] = c;
                    s_be[p] = -s;
                    s_pq[tid][0] = p;
                    s_pq[tid][1] = q;
                    s_cs[tid][0] = c;
                    s_cs[tid][1] = s;
                }
                __syncthreads();
                // H = J^T G J, entry by entry from G: column i of J is alpha_i e_i + beta_i e_partner(i)
                for (int e = tid; e < D * D; e += WG) {
                    const int i = e / D, j = e - i * D;
                    if (i > j) continue;
                    const double ai = s_al[i], bi = s_be[i], aj = s_al[j], bj = s_be[j];
                    const int pi = s_part[i], pj = s_part[j];
                    double v;
                    if (bi == 0.0 && bj == 0.0) v = G[i * CMA_LD + j];
                    else if (j == pi) v = 0.0;                 // the rotated pair's own entry
                    else v = ai * (aj * G[i * CMA_LD + j] + bj * G[i * CMA_LD + pj]) +
                             bi * (aj * G[pi * CMA_LD + j] + bj * G[pi * CMA_LD + pj]);
                    H[i * CMA_LD + j] = v;
                    H[j * CMA_LD + i] = v;
                }
                for (int e = tid; e < np * D; e += WG) {       // B <- B J: columns p, q
                    const int pr = e / D, i = e - pr * D;
                    const double c = s_cs[pr][0], s = s_cs[pr][1];
                    if (s == 0.0) continue;
                    const int p = s_pq[pr][0], q = s_pq[pr][1];
                    const double x = sB[i * CMA_LD + p], y = sB[i * CMA_LD + q];
                    sB[i * CMA_LD + p] = c * x - s * y;
                    sB[i * CMA_LD + q] = s * x + c * y;
                }
                __syncthreads();
                double* t = G;
                G = H;
                H = t;
            }
            if (tid < np) s_red[tid] = off;
            __syncthreads();
            double mx = 0.0;
            for (int i = 0; i < np; ++i) mx = fmax(mx, s_red[i]);
            converged = mx <= CMA_EIG_THRESHOLD;
            __syncthreads();
        }
        if (tid == 0 && s_code == CMA_LIVE) {
            double lo = G[0], hi = G[0];
            bool ok = converged;
            for (int i = 0; i < D; ++i) {
                const double l = G[i * CMA_LD + i];
                ok = ok && cma_finite(l) && l > 0.0;
                lo = fmin(lo, l);
                hi = fmax(hi, l);
            }
            if (!ok) s_code = CMA_EIG_BAD;
            else if (hi / lo > CMA_COND_MAX) s_code = CMA_EIG_COND;
        }
        __syncthreads();
        if (s_code == CMA_LIVE) {
            // A = (B sqrt(Lambda)) B^T, then A^-1 = (B / sqrt(Lambda)) B^T: upper tile triangle, mirrored
            for (int pass = 0; pass < 2; ++pass) {
                for (int e = tid; e < CMA_MAT; e += WG) sQ[e] = 0.0;
                __syncthreads();
                for (int e = tid; e < D * D; e += WG) {
                    const int d = e / D, k = e - d * D;
                    const double sl = sqrt(G[k * CMA_LD + k]);
                    sQ[d * CMA_LD + k] = pass == 0 ? sB[d * CMA_LD + k] * sl : sB[d * CMA_LD + k] / sl;
                }
                __syncthreads();
                double* out = (pass == 0 ? st.A : st.Ainv) + r * dd;
                cma_mm_nt(sQ, sB, DP / 16, DP / 16, DP, true, [](int, int) { return 0.0; },
                          [&](int i, int j, double v) {
                              if (i <= j && j < D) {
                                  out[(size_t)i * D + j] = v;
                                  out[(size_t)j * D + i] = v;
                              }
                          });
                __syncthreads();
            }
        }
    }
    __syncthreads();
    const int code = s_code;
    if (tid == 0) {
        st.gen[r] = g + 1;
        if (code != CMA_LIVE) {
            st.frozen[r] = code;
            atomicOr(st.flags, ROBO_FLAG_FROZEN);
        }
    }
    if (row) cma_trace_state(st, r, row, hs, code);
}

// the instance with the largest best-so-far value, first on ties -> st.out; the flag words of the candidate handle (the
// sweep's) and of the generations are reported and cleared
__global__ void cma_result_kernel(CmaState st, unsigned* __restrict__ cand_flags) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int D = st.D;
    unsigned flags = *cand_flags | *st.flags;
    *cand_flags = 0u;
    *st.flags = 0u;
    int best = -1;
    for (int r = 0; r < st.R; ++r) {
        if (st.frozen[r] == CMA_UNUSED) continue;
        if (best < 0 || st.bestf[r] > st.bestf[best]) best = r;
    }
    const double value = best >= 0 ? st.bestf[best] : __longlong_as_double(0x7FF8000000000000LL);
    if (value != value) flags |= ROBO_FLAG_NAN;
    for (int d = 0; d < D; ++d) st.out[d] = best >= 0 ? st.bestx[(size_t)best * D + d] : 0.0;
    st.out[D] = value;
    st.out[D + 1] = __longlong_as_double((long long)best);
    st.out[D + 2] = __longlong_as_double((long long)flags);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
void cma_free(CmaWork* w) {
    if (!w) return;
    hipFree(w->d_block);
    hipFree(w->d_trace);
    refine_free(w->sel);
    delete w;
}

int launch_cma_init(robo_ctx* ctx, const CmaState& st, const RefineState& sel) {
    hipLaunchKernelGGL(cma_init_kernel, dim3((unsigned)st.R), dim3(64), 0, ctx->stream, st, sel);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_cma_ask(robo_ctx* ctx, const CmaState& st, int g) {
    hipLaunchKernelGGL(cma_ask_kernel, dim3((unsigned)st.R), dim3(WG), 0, ctx->stream, st, g);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_cma_tell(robo_ctx* ctx, const CmaState& st, int g) {
    hipLaunchKernelGGL(cma_tell_kernel, dim3((unsigned)st.R), dim3(WG), 0, ctx->stream, st, g);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_cma_result(robo_ctx* ctx, const CmaState& st, unsigned* d_cand_flags) {
    hipLaunchKernelGGL(cma_result_kernel, dim3(1), dim3(64), 0, ctx->stream, st, d_cand_flags);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

}  // namespace robo
