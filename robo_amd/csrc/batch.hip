// Greedy batch proposals with fantasised picks, resident on the device (robo_acq_batch_cand, robo_acq_batch_marginal_cand;
// the reference proposes one point per model fit: robo/solver/bayesian_optimization.py:156-203).
//
//   sweep (predict.hip + acq.hip, unchanged) -> batch_init_kernel: the unfloored latent moments of every candidate
//   -> batch_record_kernel: pick 0
//   -> (q - 1) x [ per hyper-parameter sample: batch_kstar_kernel (k_*(x_j), the fantasy target, eta)
//                  -> forward / backward block rows (beta_j = K^-1 k_*(x_j)) -> batch_cond_kernel (rank-one conditioning
//                  of every candidate + acquisition) ;  the sweep's final reduction (acq.hip) ; batch_record_kernel ]
//
// The rule (include/robo_hip.h): after pick j at x_j with fantasy target y_f, every candidate's LATENT moments (the scale
// the factor lives in, before the output transform, never floored) are conditioned on (x_j, y_f) observed with the
// model's noise, at FIXED theta, constant mean and output transform:
//     c(x) = k(x, x_j) - k_*(x)^T beta_j - sum_{t < j} c_t(x) c_t(x_j) / d_t      (beta_j = K^-1 k_*(x_j), K the fitted gram)
//     d = var_lat(x_j) + noise                                                   (noise: the diagonal term of the fit)
//     var_lat(x) -= c(x)^2 / d                  mu_lat(x) += c(x) (y_f - mu(x_j)) / d
// which is what appending (x_j, y_f) and refitting with everything else frozen gives.  The transform and the DBL_EPSILON
// floor are applied where the sweep applies them: when the acquisition is formed.
//
// beta_j always comes from the two triangular solves with the factor and its inverted diagonal blocks, never from the
// explicit inverse W: a result cannot depend on the winv_cond_max guard or on whether W exists.  The conditioning pass
// generates k(x, X_n) in registers and writes no cross-gram tile; it needs no solve workspace.
//
// Ordering is the stream's alone: the winner's index stays in device memory (BatchState::idx) and the next pick's
// kernels read x_j from the candidate buffer through it.  Every sum has a fixed order that does not depend on the grid.
#include "api_internal.h"
#include "batch_cond.h"

namespace robo {

__device__ __forceinline__ double batch_nan() { return __longlong_as_double(0x7FF8000000000000LL); }

// everything the picks start from; one launch per sample right after that sample's posterior (d_q / d_mu / d_mean / d_var
// of the candidate handle still hold it)
__global__ __launch_bounds__(256) void batch_init_kernel(BatchState st, int s, const double* __restrict__ q,
                                                         const double* __restrict__ mu, const double* __restrict__ mean,
                                                         const double* __restrict__ var, const double* __restrict__ Xc,
                                                         const double* __restrict__ ism, CovParams cp, double mean_c,
                                                         double eta) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) st.eta[s] = eta;
    if (i >= st.m) return;
    const size_t at = (size_t)s * st.m_pad + i;
    const double u = Xc[i * cp.dim + cp.dim - 1] * ism[cp.dim - 1];
    st.mu_lat[at] = mu[i] + mean_c;
    st.var_lat[at] = cov_self(cp, u) - q[i];
    st.mean_t[at] = mean[i];
    if (st.trace) {
        double* row = st.trace + ((size_t)s * st.m + i) * 2;       // pick 0
        row[0] = mean[i];
        row[1] = var[i];
    }
}

// outputs of a call: "no pick" everywhere
__global__ __launch_bounds__(256) void batch_reset_kernel(BatchState st) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < st.q) {
        st.idx[t] = -1;
        st.val[t] = batch_nan();
        st.flg[t] = 0u;
    }
    if (t < st.q * st.S) st.fant[t] = batch_nan();
    if (t == 0) {
        *st.n_made = 0;
        *st.stop = 0;
    }
}

// pick j := the reduction's winner.  A NaN winner is recorded and ends the selection.  cand_flags: the sweep's flag word
// (pick 0: reported and cleared, as the sweep's own read-back does), nullptr for the later picks, whose conditioning
// pass raises its flags in st.flg[j] directly.
__global__ void batch_record_kernel(BatchState st, int j, const double* __restrict__ best_val,
                                    const long long* __restrict__ best_idx, unsigned* __restrict__ cand_flags) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (*st.stop) return;
    const double v = *best_val;
    st.val[j] = v;
    st.idx[j] = *best_idx;
    if (cand_flags) {
        st.flg[j] = *cand_flags;
        *cand_flags = 0u;
    }
    *st.n_made = j + 1;
    if (v != v) *st.stop = 1;
}

// k_*(x_j) of sample s into st.w (rows >= n: 0), and the scalars of this conditioning step: the fantasy target, d,
// the gain (y_f - mu(x_j)) / d in the latent scale (exactly 0 for the kriging believer: its mean state is never touched),
// eta := min(eta, y_f)
__global__ __launch_bounds__(256) void batch_kstar_kernel(BatchState st, int s, int j, const double* __restrict__ Xc,
                                                          const double* __restrict__ Xs, const double* __restrict__ ism,
                                                          CovParams cp, int n, int n_pad, double noise, double y_mean,
                                                          double y_std, int fantasy_kind, double liar) {
    __shared__ double sJ[MAX_DIM];
    if (*st.stop) return;
    const int D = cp.dim;
    const long long pj = st.idx[j - 1];
    for (int d = threadIdx.x; d < D; d += 256) sJ[d] = Xc[pj * D + d] * ism[d];
    __syncthreads();
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < n_pad) st.w[(size_t)s * n_pad + r] = r < n ? cov_rows(cp, sJ, Xs + (size_t)r * D) : 0.0;
    if (r == 0) {
        const size_t at = (size_t)s * st.m_pad + pj;
        const double d = st.var_lat[at] + noise;
        const bool believer = fantasy_kind == ROBO_FANTASY_KRIGING_BELIEVER;
        const double yf = believer ? st.mean_t[at] : liar;
        const double gain = believer ? 0.0 : ((yf - y_mean) / y_std - st.mu_lat[at]) / d;
        st.fant[(size_t)(j - 1) * st.S + s] = yf;
        st.scal[2 * s] = d;
        st.dhist[(size_t)s * st.qcap + (j - 1)] = d;
        st.scal[2 * s + 1] = gain;
        const double e = st.eta[s];
        st.eta[s] = yf < e ? yf : e;
    }
}

// ---- beta = L^-T L^-1 k_*: one right-hand side, block rows of 128 with the fit's inverted diagonal blocks -------------
// The MFMA block-row substitution of predict.hip works on tiles of 128 right-hand sides; with ONE it would spend 127 / 128
// of its products on padding (2 GFLOP on one CU at N = 4096).  The same recurrence on a vector is bound by reading L once
// per direction (67 MB at N = 4096), so it is written as matrix-vector products:
//   forward, step i:   v_i = Linv_ii w_i ;  w_j -= L[j, i] v_i   for the block rows j > i   (one workgroup per j)
//   backward, step i:  b_i = Linv_ii^T v_i ;  v_j -= L[i, j]^T b_i   for the block columns j < i
// Every workgroup of a step forms the 128-entry diagonal solve itself (128 KB out of L2) instead of waiting for another
// one: a launch boundary per step is the only ordering.  Block i is final when its step starts and no workgroup of the
// step writes it.  Rows >= n (the augmented row, the padding) take no part.
__global__ __launch_bounds__(256) void batch_fwd_kernel(const double* __restrict__ L, int ld, const double* __restrict__ Linv,
                                                        double* __restrict__ w, double* __restrict__ v, int i, int n,
                                                        const int* __restrict__ stop) {
    __shared__ double sw[NB], sv[NB];
    if (*stop) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nv = n - i * NB < NB ? n - i * NB : NB;
    if (tid < NB) sw[tid] = tid < nv ? w[i * NB + tid] : 0.0;
    __syncthreads();
    const double* Li = Linv + (size_t)i * NB * NB;
    for (int r = wave * 32; r < wave * 32 + 32; ++r) {
        double a = 0.0;
        if (r < nv) {
            a = Li[r * NB + lane] * sw[lane];
            a = fma(Li[r * NB + 64 + lane], sw[64 + lane], a);
        }
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        if (lane == 0) sv[r] = a;
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid < NB) v[i * NB + tid] = sv[tid];
    const int jb = i + 1 + blockIdx.x;                      // the block row this workgroup updates
    if (jb * NB >= n) return;
    const double v0 = sv[lane], v1 = sv[64 + lane];
    for (int r = wave * 32; r < wave * 32 + 32; ++r) {
        const int row = jb * NB + r;
        double a = 0.0;
        if (row < n) {
            const double* Lr = L + (size_t)row * ld + (size_t)i * NB;
            a = Lr[lane] * v0;
            a = fma(Lr[64 + lane], v1, a);
        }
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        if (lane == 0 && row < n) w[row] -= a;
    }
}

__global__ __launch_bounds__(256) void batch_bwd_kernel(const double* __restrict__ L, int ld, const double* __restrict__ Linv,
                                                        double* __restrict__ v, double* __restrict__ beta, int i, int n,
                                                        const int* __restrict__ stop) {
    __shared__ double sv[NB], sb[NB], sp[NB];
    if (stop && *stop) return;
    const int tid = threadIdx.x, c = tid & (NB - 1), half = tid >> 7;
    const int nv = n - i * NB < NB ? n - i * NB : NB;
    if (tid < NB) sv[tid] = tid < nv ? v[i * NB + tid] : 0.0;
    __syncthreads();
    const double* Li = Linv + (size_t)i * NB * NB;
    double a = 0.0;
    for (int r = half * 64; r < half * 64 + 64; ++r)
        if (r < nv && r >= c) a = fma(Li[r * NB + c], sv[r], a);
    if (half == 1) sp[c] = a;
    __syncthreads();
    if (half == 0) sb[c] = c < nv ? a + sp[c] : 0.0;
    __syncthreads();
    if (blockIdx.x == 0 && tid < NB) beta[i * NB + tid] = sb[tid];
    const int jb = blockIdx.x;                              // the block column this workgroup updates
    if (jb >= i) return;
    a = 0.0;
    for (int r = half * 64; r < half * 64 + 64; ++r)
        if (r < nv) a = fma(L[(size_t)(i * NB + r) * ld + (size_t)jb * NB + c], sb[r], a);
    __syncthreads();
    if (half == 1) sp[c] = a;
    __syncthreads();
    if (half == 0) v[jb * NB + c] -= a + sp[c];
}

// ---- the fused conditioning pass ----------------------------------------------------------------------------------------
// k_*(x)^T beta of a workgroup's 64 candidates by the shared tile loop (batch_cond.h).
// Then lane by lane: c, the update of (mu_lat, var_lat) in memory, transform + floor, the acquisition as acq_kernel
// forms it, accumulated over the samples in sample order.  The reduction over the candidates is the sweep's own
// (launch_argmax, acq.hip).
template <int KIND, bool SMALLD>
__global__ __launch_bounds__(256) void batch_cond_kernel(BatchState st, int s, int j, const double* __restrict__ Xc,
                                                         const double* __restrict__ Xs, const double* __restrict__ ism,
                                                         CovParams cp, int n, int n_pad, double y_mean, double y_std,
                                                         int acq_kind, double par, int fantasy_kind,
                                                         double* __restrict__ acq_sum) {
    __shared__ double sX[16 * BC_LD];
    __shared__ double sB[NB];
    __shared__ double sJ[MAX_DIM];
    __shared__ double sP[4][BC_CAND];
    if (*st.stop) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, D = cp.dim;
    const long long i = (long long)blockIdx.x * BC_CAND + lane;
    const bool live = i < st.m;
    const long long ii = live ? i : 0;
    const long long pj = st.idx[j - 1];
    for (int d = tid; d < D; d += 256) sJ[d] = Xc[pj * D + d] * ism[d];
    const double dot = cond_kstar_dot<KIND, SMALLD>(Xc, Xs, ism, cp, n, st.beta + (size_t)s * n_pad, ii, sX, sB);
    sP[wave][lane] = dot;
    __syncthreads();
    if (wave != 0 || !live) return;
    const double ktb = (sP[0][lane] + sP[1][lane]) + (sP[2][lane] + sP[3][lane]);
    const double c = cond_cov<KIND>(Xc, ism, cp, sJ, ktb, i, pj, j - 1, st.chist + (size_t)s * st.qcap * st.m_pad,
                                    st.dhist + (size_t)s * st.qcap, st.m_pad);
    st.chist[((size_t)s * st.qcap + (j - 1)) * st.m_pad + i] = c;

    const size_t at = (size_t)s * st.m_pad + i;
    const double dd = st.scal[2 * s], gain = st.scal[2 * s + 1], eta = st.eta[s];
    const double vl = st.var_lat[at] - c * c / dd;
    st.var_lat[at] = vl;
    double mt;
    if (fantasy_kind == ROBO_FANTASY_KRIGING_BELIEVER) {
        mt = st.mean_t[at];                       // innovation exactly 0: the mean state is not rewritten
    } else {
        const double ml = st.mu_lat[at] + c * gain;
        st.mu_lat[at] = ml;
        mt = ml * y_std + y_mean;
        st.mean_t[at] = mt;
    }
    double vt = vl * (y_std * y_std);
    const double eps = 2.220446049250313e-16;
    vt = vt < eps ? eps : vt;                     // np.clip(var, eps, inf); NaN propagates like np.clip
    if (st.trace) {
        double* row = st.trace + (((size_t)j * st.S + s) * st.m + i) * 2;
        row[0] = mt;
        row[1] = vt;
    }
    unsigned f = 0;
    double a;
    if (acq_kind == ROBO_ACQ_EI) {
        a = acq_ei(mt, vt, eta, par);
        if (a < 0.0 && a > -2.2250738585072014e-308) a = 0.0;    // as acq_kernel
        if (a < 0.0) f |= ROBO_FLAG_NEGATIVE_EI;
    } else if (acq_kind == ROBO_ACQ_LOG_EI) {
        a = acq_log_ei(mt, vt, eta, par);
    } else if (acq_kind == ROBO_ACQ_PI) {
        a = acq_pi(mt, vt, eta, par);
    } else {
        a = acq_lcb(mt, vt, par);
    }
    if (sqrt(vt) == 0.0) f |= ROBO_FLAG_ZERO_SIGMA;
    if (isnan(a)) f |= ROBO_FLAG_NAN;
    if (f != 0) atomicOr(&st.flg[j], f);
    if (s == 0) acq_sum[i] = a;
    else acq_sum[i] += a;
}

// ---- host side ------------------------------------------------------------------------------------------------------------
int batch_alloc(robo_ctx* ctx, int64_t m, int64_t m_pad, int S, int n_pad, int q, BatchWork** out) {
    BatchWork* w = new BatchWork();
    w->m = m;
    w->S = S;
    w->n_pad = n_pad;
    w->q = q;
    BatchState& st = w->st;
    const size_t sm = (size_t)S * m_pad, sn = (size_t)S * n_pad;
    BlockLayout lay(16);
    lay.add(&st.mu_lat, sm);
    lay.add(&st.var_lat, sm);
    lay.add(&st.mean_t, sm);
    lay.add(&st.w, sn);
    lay.add(&st.v, sn);
    lay.add(&st.beta, sn);
    lay.add(&st.chist, (size_t)S * q * m_pad);
    lay.add(&st.dhist, (size_t)S * q);
    lay.add(&st.scal, (size_t)2 * S);
    lay.add(&st.eta, (size_t)S);
    // everything a call reports (values, fantasies, indices, flags, picks made) is one contiguous range from `val` to the
    // end of the block: ONE copy into pinned memory, as the sweep's own report
    w->rep_off = lay.add(&st.val, (size_t)q);
    w->off_fant = lay.add(&st.fant, (size_t)q * S) - w->rep_off;
    w->off_idx = lay.add(&st.idx, (size_t)q) - w->rep_off;
    w->off_flg = lay.add(&st.flg, (size_t)q) - w->rep_off;
    w->off_int = lay.add(&st.n_made, 4) - w->rep_off;         // [n_made, stop] and padding
    w->rep_bytes = lay.bytes() - w->rep_off;
    if (hipMalloc((void**)&w->d_block, lay.bytes()) != hipSuccess) {
        set_error("hipMalloc of %zu bytes failed (batch selection state)", lay.bytes());
        delete w;
        return ROBO_RUNTIME_ERROR;
    }
    if (hipHostMalloc((void**)&w->h_report, w->rep_bytes) != hipSuccess) {
        set_error("hipHostMalloc of %zu bytes failed (batch selection report)", w->rep_bytes);
        hipFree(w->d_block);
        delete w;
        return ROBO_RUNTIME_ERROR;
    }
    lay.bind(w->d_block);
    st.stop = st.n_made + 1;
    st.S = S;
    st.q = q;
    st.qcap = q;
    st.m = m;
    st.m_pad = m_pad;
    (void)ctx;
    *out = w;
    return ROBO_OK;
}

void batch_free(BatchWork* w) {
    if (!w) return;
    hipFree(w->d_block);
    hipFree(w->d_trace);
    if (w->h_report) hipHostFree(w->h_report);
    delete w;
}

int launch_batch_reset(robo_ctx* ctx, const BatchState& st) {
    hipLaunchKernelGGL(batch_reset_kernel, dim3((unsigned)((st.q * st.S + 255) / 256)), dim3(256), 0, ctx->stream, st);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_batch_init(robo_gp* gp, const BatchState& st, const robo_cand* cand, int s, double eta) {
    hipLaunchKernelGGL(batch_init_kernel, dim3((unsigned)((st.m + 255) / 256)), dim3(256), 0, gp->ctx->stream, st, s,
                       (const double*)cand->d_q, (const double*)cand->d_mu, (const double*)cand->d_mean,
                       (const double*)cand->d_var, (const double*)cand->d_Xc, (const double*)gp->d_theta, gp->cov,
                       gp->mean_c, eta);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_batch_record(robo_ctx* ctx, const BatchState& st, const robo_cand* cand, int j, bool take_flags) {
    hipLaunchKernelGGL(batch_record_kernel, dim3(1), dim3(64), 0, ctx->stream, st, j,
                       (const double*)(cand->d_part_val + cand->n_part), (const long long*)(cand->d_part_idx + cand->n_part),
                       take_flags ? cand->d_flags : nullptr);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_fwd_rows(robo_gp* gp, double* d_w, double* d_v, const int* d_stop) {
    const int n = gp->n, n_pad = gp->n_pad, nbk = (n + NB - 1) / NB;
    for (int i = 0; i < nbk; ++i)
        hipLaunchKernelGGL(batch_fwd_kernel, dim3((unsigned)(nbk - 1 - i > 1 ? nbk - 1 - i : 1)), dim3(256), 0,
                           gp->ctx->stream, (const double*)gp->d_K, n_pad, (const double*)gp->d_Linv, d_w, d_v, i, n, d_stop);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_bwd_rows(robo_gp* gp, double* d_v, double* d_beta, const int* d_stop) {
    const int n = gp->n, n_pad = gp->n_pad, nbk = (n + NB - 1) / NB;
    for (int i = nbk - 1; i >= 0; --i)
        hipLaunchKernelGGL(batch_bwd_kernel, dim3((unsigned)(i > 1 ? i : 1)), dim3(256), 0, gp->ctx->stream,
                           (const double*)gp->d_K, n_pad, (const double*)gp->d_Linv, d_v, d_beta, i, n, d_stop);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

// one conditioning step of sample s for pick j >= 1: k_*(x_j) and the scalars, beta, the pass over the candidates
int launch_batch_condition(robo_gp* gp, const BatchState& st, const robo_cand* cand, int s, int j, int acq_kind, double par,
                           int fantasy_kind, double liar) {
    hipStream_t stream = gp->ctx->stream;
    const int n = gp->n, n_pad = gp->n_pad;
    const double* Xc = cand->d_Xc;
    const double* Xs = gp->d_Xs;
    const double* ism = gp->d_theta;
    double* w = st.w + (size_t)s * n_pad;
    double* v = st.v + (size_t)s * n_pad;
    double* beta = st.beta + (size_t)s * n_pad;
    hipLaunchKernelGGL(batch_kstar_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, stream, st, s, j, Xc, Xs, ism,
                       gp->cov, n, n_pad, gp->noise, gp->y_mean, gp->y_std, fantasy_kind, liar);
    ROBO_TRY(launch_fwd_rows(gp, w, v, st.stop));
    ROBO_TRY(launch_bwd_rows(gp, v, beta, st.stop));
    const dim3 grid((unsigned)((st.m + BC_CAND - 1) / BC_CAND));
#define ROBO_COND_CALL(KIND)                                                                                              \
    do {                                                                                                                  \
        if (gp->dim <= 16)                                                                                                \
            hipLaunchKernelGGL((batch_cond_kernel<KIND, true>), grid, dim3(256), 0, stream, st, s, j, Xc, Xs, ism, gp->cov, n, \
                               n_pad, gp->y_mean, gp->y_std, acq_kind, par, fantasy_kind, cand->d_acq_sum);               \
        else                                                                                                              \
            hipLaunchKernelGGL((batch_cond_kernel<KIND, false>), grid, dim3(256), 0, stream, st, s, j, Xc, Xs, ism, gp->cov, n, \
                               n_pad, gp->y_mean, gp->y_std, acq_kind, par, fantasy_kind, cand->d_acq_sum);               \
    } while (0)
    if (gp->kind == ROBO_KERNEL_MATERN52_ARD) ROBO_COND_CALL(ROBO_KERNEL_MATERN52_ARD);
    else if (gp->kind == ROBO_KERNEL_RBF_ARD) ROBO_COND_CALL(ROBO_KERNEL_RBF_ARD);
    else ROBO_COND_CALL(ROBO_KERNEL_FABOLAS);
#undef ROBO_COND_CALL
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

// ---- the driver ---------------------------------------------------------------------------------------------------------------
static int select_ensure(robo_gp* g, const robo_cand* k, int S, int q, BatchWork** out) {
    BatchWork* w = g->batch;
    if (w && (w->m != k->m || w->S != S || w->n_pad < g->n_pad || w->q < q)) {
        ROBO_HIP_CHECK(hipStreamSynchronize(g->ctx->stream));
        batch_free(w);
        g->batch = w = nullptr;
    }
    if (!w) ROBO_TRY(batch_alloc(g->ctx, k->m, k->m_pad, S, g->n_pad_max, q, &g->batch));
    *out = g->batch;
    return ROBO_OK;
}

// marginal: pick 0 is robo_acq_eval_marginal_cand's sweep (accumulate, divide); otherwise robo_acq_eval_cand's
static int batch_core(robo_gp* const* gps, int32_t S, bool marginal, int32_t acq_kind, double par, const double* etas,
                      robo_cand* k, int32_t q, int32_t fantasy_kind, double liar, int64_t* out_idx, double* out_values,
                      double* out_fantasy, uint32_t* out_flags, int32_t* out_n_made, double* out_trace) {
    if (!gps || S < 1 || !etas || !k || !out_idx) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(check_acq_kind(acq_kind));
    if (q < 1 || (int64_t)q > k->m || q > BATCH_MAX_Q) {
        set_error("batch selection: q = %d outside 1 .. min(m = %lld, %d)", q, (long long)k->m, BATCH_MAX_Q);
        return ROBO_BAD_ARGUMENT;
    }
    if (fantasy_kind != ROBO_FANTASY_KRIGING_BELIEVER && fantasy_kind != ROBO_FANTASY_CONSTANT_LIAR) {
        set_error("unknown fantasy kind %d", fantasy_kind);
        return ROBO_BAD_ARGUMENT;
    }
    ROBO_TRY(ensemble_check("batch selection", ENSEMBLE_ONE_KIND_FP64, gps, S, k));
    robo_gp* g0 = gps[0];
    robo_ctx* c = g0->ctx;
    BatchWork* w = nullptr;
    ROBO_TRY(select_ensure(g0, k, S, q, &w));
    const size_t trace_len = (size_t)q * S * k->m * 2;
    if (out_trace) ROBO_TRY(dev_grow(c->stream, &w->d_trace, &w->trace_cap, trace_len));
    w->st.q = q;
    w->st.trace = out_trace ? w->d_trace : nullptr;
    const BatchState& st = w->st;
    const bool state = q > 1 || out_trace;        // q = 1: the sweep alone

    // pick 0: the sweep, launch for launch; every sample's latent moments are taken while its posterior is in the handle
    ROBO_TRY(launch_batch_reset(c, st));
    for (int s = 0; s < S; ++s) {
        ROBO_TRY(clear_flags_on_error(k, predict_core(gps[s], k)));
        ROBO_TRY(clear_flags_on_error(k, launch_acq(c, k, acq_kind, par, etas[s], marginal, s == 0)));
        if (state) ROBO_TRY(clear_flags_on_error(k, launch_batch_init(gps[s], st, k, s, etas[s])));
    }
    if (marginal) ROBO_TRY(clear_flags_on_error(k, launch_argmax(k, k->d_acq_sum, (double)S)));
    int status = launch_batch_record(c, st, k, 0, true);
    // the later picks: launches only, ordered by the stream
    for (int j = 1; status == ROBO_OK && j < q; ++j) {
        for (int s = 0; status == ROBO_OK && s < S; ++s)
            status = launch_batch_condition(gps[s], st, k, s, j, acq_kind, par, fantasy_kind, liar);
        if (status == ROBO_OK) status = launch_argmax(k, k->d_acq_sum, marginal ? (double)S : 1.0);
        if (status == ROBO_OK) status = launch_batch_record(c, st, k, j, false);
    }
    // read-back: one copy of the report range into pinned memory (+ the trace, diagnostics), the one synchronisation
    ROBO_TRY(finish_call(k, "batch selection", status, {{w->h_report, w->d_block + w->rep_off, w->rep_bytes},
                                                        {out_trace, w->d_trace, trace_len * sizeof(double)}}));
    const double* hv = reinterpret_cast<const double*>(w->h_report);
    const long long* hi = reinterpret_cast<const long long*>(w->h_report + w->off_idx);
    const unsigned* hf = reinterpret_cast<const unsigned*>(w->h_report + w->off_flg);
    for (int j = 0; j < q; ++j) {
        out_idx[j] = (int64_t)hi[j];
        if (out_values) out_values[j] = hv[j];
        if (out_flags) out_flags[j] = hf[j];
    }
    if (out_fantasy) memcpy(out_fantasy, w->h_report + w->off_fant, (size_t)q * S * sizeof(double));
    int made = 0;
    memcpy(&made, w->h_report + w->off_int, sizeof(int));
    if (out_n_made) *out_n_made = made;
    return ROBO_OK;
}

}  // namespace robo

using namespace robo;

extern "C" {

int32_t robo_acq_batch_cand(robo_gp* g, int32_t acq_kind, double par, double eta, robo_cand* k, int32_t q,
                            int32_t fantasy_kind, double liar, int64_t* out_idx, double* out_values, double* out_fantasy,
                            uint32_t* out_flags, int32_t* out_n_made, double* out_trace) {
    return batch_core(&g, g ? 1 : 0, false, acq_kind, par, &eta, k, q, fantasy_kind, liar, out_idx, out_values, out_fantasy,
                      out_flags, out_n_made, out_trace);
}

int32_t robo_acq_batch_marginal_cand(robo_gp* const* gps, int32_t S, int32_t acq_kind, double par, const double* etas,
                                     robo_cand* k, int32_t q, int32_t fantasy_kind, double liar, int64_t* out_idx,
                                     double* out_values, double* out_fantasy, uint32_t* out_flags, int32_t* out_n_made,
                                     double* out_trace) {
    return batch_core(gps, S, true, acq_kind, par, etas, k, q, fantasy_kind, liar, out_idx, out_values, out_fantasy,
                      out_flags, out_n_made, out_trace);
}

}  // extern "C"
