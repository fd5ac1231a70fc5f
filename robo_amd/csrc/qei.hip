// Joint Monte-Carlo batch EI with greedy picks, resident on the device (robo_qei_batch_cand, robo_qei_batch_marginal_cand;
// no counterpart in the reference, which proposes one point per model fit).
//
//   sweep (predict.hip + acq.hip, unchanged) -> batch_init_kernel -> qei_scen_kernel (b^k := eta - par) -> batch_record_kernel
//   -> (q - 1) x [ per hyper-parameter sample: qei_kstar_kernel (k_*(p_t), d_t) -> forward / backward block rows (beta_t)
//                  -> qei_scen_kernel (f^k(p_t), b^k) -> qei_cond_kernel (c_t(x), the residual variance)
//                  -> qei_fold_kernel (K terms of EI per candidate) ;  the sweep's final reduction ; batch_record_kernel ]
//
// The rule (include/robo_hip.h): qEI(x_0 .. x_{q-1}) = E[(eta - par - min_t f(x_t))^+] under the joint posterior.  With
// b^k = min(eta - par, f^k(picks so far)) in scenario k,  qEI(picks, x) = qEI(picks) + E[(b - f(x))^+]: a pick maximises the
// increment.  The picks are conditioned on as LATENT values (no noise, no fantasy target): c_t(x) and the pivots d_t that
// batch.hip's machinery keeps are the rows of the Cholesky factor of the joint covariance of (picks, candidate), so in
// scenario k the candidate's mean is shifted by y_std sum_u l_u(x) z[k][u], l_u = c_u / sqrt(d_u), its variance is the
// residual one, and the innermost normal is integrated in closed form: a term is acq_ei (kern_math.h).
//
// The state is a BatchState of its own (batch.hip's reset / init / record kernels and block-row solves run on it unchanged;
// its mean state is never touched and its `fant` slots report d_t) plus the scenarios' block (z, b).  Ordering is the
// stream's alone; every sum has a fixed order that depends on nothing but K and the pick's number.
#include <cmath>

#include "api_internal.h"
#include "batch_cond.h"

namespace robo {

static_assert(QEI_MAX_Q == ROBO_QEI_MAX_Q && QEI_MAX_K == ROBO_QEI_MAX_K, "the limits of include/robo_hip.h");
constexpr int QF_ZK = 8;             // scenarios per wave whose z rows are staged at a time (fold kernel)

// k_*(p_t) of sample s into st.w (rows >= n: 0), t = j - 1, and the pivot d_t = max(var_lat(p_t), dfloor): no noise term and
// no jitter, a pick is not an observation.  NaN propagates.
__global__ __launch_bounds__(256) void qei_kstar_kernel(BatchState st, int s, int j, const double* __restrict__ Xc,
                                                        const double* __restrict__ Xs, const double* __restrict__ ism,
                                                        CovParams cp, int n, int n_pad, double dfloor) {
    __shared__ double sJ[MAX_DIM];
    if (*st.stop) return;
    const int D = cp.dim;
    const long long pj = st.idx[j - 1];
    for (int d = threadIdx.x; d < D; d += 256) sJ[d] = Xc[pj * D + d] * ism[d];
    __syncthreads();
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < n_pad) st.w[(size_t)s * n_pad + r] = r < n ? cov_rows(cp, sJ, Xs + (size_t)r * D) : 0.0;
    if (r == 0) {
        const double v = st.var_lat[(size_t)s * st.m_pad + pj];
        const double d = v < dfloor ? dfloor : v;
        st.fant[(size_t)(j - 1) * st.S + s] = d;
        st.scal[2 * s] = d;
        st.dhist[(size_t)s * st.qcap + (j - 1)] = d;
    }
}

// The K scenarios of sample s.  j == 0: b^k := b0 (eta_s - par).  j >= 1, after pick t = j - 1 at p_t and its pivot:
//     f^k(p_t) = mean_t(p_t) + y_std (sum_{u < t} l_u(p_t) z[k][u] + sqrt(d_t) z[k][t]),   b^k := min(b^k, f^k(p_t))
// (u ascending, every product fused into the sum; a NaN f^k makes b^k NaN, as np.minimum).  One workgroup.
__global__ __launch_bounds__(256) void qei_scen_kernel(BatchState st, QeiState qs, int s, int j, double y_std, double b0) {
    __shared__ double sl[QEI_MAX_Q];
    const int K = qs.K;
    double* b = qs.b + (size_t)s * K;
    double* best = qs.best ? qs.best + ((size_t)j * st.S + s) * K : nullptr;
    if (j == 0) {
        for (int k = threadIdx.x; k < K; k += 256) {
            b[k] = b0;
            if (best) best[k] = b0;
        }
        return;
    }
    if (*st.stop) return;
    const int t = j - 1;
    const long long p = st.idx[t];
    const double* dh = st.dhist + (size_t)s * st.qcap;
    if ((int)threadIdx.x < t) sl[threadIdx.x] = st.chist[((size_t)s * st.qcap + threadIdx.x) * st.m_pad + p] / sqrt(dh[threadIdx.x]);
    __syncthreads();
    const double sd = sqrt(dh[t]), mean = st.mean_t[(size_t)s * st.m_pad + p];
    for (int k = threadIdx.x; k < K; k += 256) {
        const double* zk = qs.z + (size_t)k * st.q;
        double acc = 0.0;
        for (int u = 0; u < t; ++u) acc = fma(sl[u], zk[u], acc);
        acc = fma(sd, zk[t], acc);
        const double f = fma(y_std, acc, mean);
        double bk = b[k];
        if (f < bk || f != f) bk = f;
        b[k] = bk;
        if (best) best[k] = bk;
    }
}

// The conditioning pass on the latent value at p_t, t = j - 1: batch_cond_kernel's tile loop (batch_cond.h), then lane by lane
//     c_t(x) = k(x, p_t) - k_*(x)^T beta_t - sum_{u < t} c_u(x) c_u(p_t) / d_u,   l = c_t(x) / sqrt(d_t),   var_lat(x) -= l^2
// The mean state is not touched.  The trace row of pick j: the transformed mean, the transformed, floored residual variance.
template <int KIND, bool SMALLD>
__global__ __launch_bounds__(256) void qei_cond_kernel(BatchState st, QeiState qs, int s, int j, const double* __restrict__ Xc,
                                                       const double* __restrict__ Xs, const double* __restrict__ ism,
                                                       CovParams cp, int n, int n_pad, double y_std) {
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
    if (qs.coef) qs.coef[((size_t)(j - 1) * st.S + s) * st.m + i] = c;
    const size_t at = (size_t)s * st.m_pad + i;
    const double l = c / sqrt(st.scal[2 * s]);
    const double vl = st.var_lat[at] - l * l;
    st.var_lat[at] = vl;
    if (st.trace) {
        double vt = vl * (y_std * y_std);
        const double eps = 2.220446049250313e-16;
        vt = vt < eps ? eps : vt;
        double* row = st.trace + (((size_t)j * st.S + s) * st.m + i) * 2;
        row[0] = st.mean_t[at];
        row[1] = vt;
    }
}

// ---- the fold ---------------------------------------------------------------------------------------------------------------
// g_s(x) = (1 / K) sum_k acq_ei(mean_t(x) + y_std sum_{u < j} l_u(x) z[k][u], max(var_lat(x) y_std^2, eps), b^k, 0)
// A workgroup owns 64 candidates, one per lane; its l_u(x) = c_u(x) / sqrt(d_u) (u < j, from the history) sit in LDS as
// [u][lane].  The K terms go in FOUR groups of ceil(K / 4) consecutive scenarios, one per wave (group w: k = w ceil(K / 4)
// ...), each summed with k ascending from +0; g = ((G0 + G1) + (G2 + G3)) / K.  The grouping depends on K alone.  b^k and,
// QF_ZK scenarios per wave at a time, the rows z[k][0 .. j) are staged in LDS and read as broadcasts.  Per term the inner
// sum runs over u ascending with fused products, and the shifted mean is one fma.  A term in (-DBL_MIN, 0) counts as +0 and
// a negative one raises ROBO_FLAG_NEGATIVE_EI, as in acq_kernel; ZERO_SIGMA / NAN as there.  Accumulated over the samples
// in sample order like batch_cond_kernel.  Dynamic LDS: (64 j + 4 QF_ZK j + K + 256 + j) doubles, at most 57.8 KB.
__global__ __launch_bounds__(256) void qei_fold_kernel(BatchState st, QeiState qs, int s, int j, double y_std,
                                                       double* __restrict__ acq_sum) {
    HIP_DYNAMIC_SHARED(double, sm)
    if (*st.stop) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, K = qs.K, Kq = (K + 3) / 4, q = st.q;
    double* sL = sm;                          // [j][64]
    double* sZ = sL + j * 64;                 // [4][QF_ZK][j]
    double* sb = sZ + 4 * QF_ZK * j;          // [K]
    double* sP = sb + K;                      // [4][64]
    double* sD = sP + 256;                    // [j]
    const long long i0 = (long long)blockIdx.x * 64, i = i0 + lane;
    const bool live = i < st.m;
    if (tid < j) sD[tid] = sqrt(st.dhist[(size_t)s * st.qcap + tid]);
    for (int k = tid; k < K; k += 256) sb[k] = qs.b[(size_t)s * K + k];
    __syncthreads();
    for (int e = tid; e < j * 64; e += 256) {
        const int u = e >> 6;
        const long long x = i0 + (e & 63);
        sL[e] = x < st.m ? st.chist[((size_t)s * st.qcap + u) * st.m_pad + x] / sD[u] : 0.0;
    }
    const size_t at = (size_t)s * st.m_pad + (live ? i : 0);
    const double mean = st.mean_t[at];
    double vt = st.var_lat[at] * (y_std * y_std);
    const double eps = 2.220446049250313e-16;
    vt = vt < eps ? eps : vt;                 // np.clip(var, eps, inf); NaN propagates like np.clip
    unsigned f = 0;
    double sum = 0.0;
    for (int k0 = 0; k0 < Kq; k0 += QF_ZK) {
        __syncthreads();
        for (int e = tid; e < 4 * QF_ZK * j; e += 256) {
            const int w = e / (QF_ZK * j), rem = e - w * (QF_ZK * j), kk = rem / j, u = rem - kk * j;
            const int kl = k0 + kk, k = w * Kq + kl;
            sZ[e] = (kl < Kq && k < K) ? qs.z[(size_t)k * q + u] : 0.0;
        }
        __syncthreads();
        if (live) {
            for (int kk = 0; kk < QF_ZK; ++kk) {
                const int kl = k0 + kk, k = wave * Kq + kl;
                if (kl >= Kq || k >= K) break;
                const double* zk = sZ + (wave * QF_ZK + kk) * j;
                double acc = 0.0;
                for (int u = 0; u < j; ++u) acc = fma(sL[u * 64 + lane], zk[u], acc);
                double a = acq_ei(fma(y_std, acc, mean), vt, sb[k], 0.0);
                if (a < 0.0 && a > -2.2250738585072014e-308) a = 0.0;    // as acq_kernel
                if (a < 0.0) f |= ROBO_FLAG_NEGATIVE_EI;
                sum += a;
            }
        }
    }
    sP[wave * 64 + lane] = sum;
    __syncthreads();
    if (live && wave == 0) {
        const double g = ((sP[lane] + sP[64 + lane]) + (sP[128 + lane] + sP[192 + lane])) / (double)K;
        if (sqrt(vt) == 0.0) f |= ROBO_FLAG_ZERO_SIGMA;
        if (isnan(g)) f |= ROBO_FLAG_NAN;
        if (s == 0) acq_sum[i] = g;
        else acq_sum[i] += g;
    }
    if (live && f != 0) atomicOr(&st.flg[j], f);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
static int qei_alloc(robo_ctx* ctx, const robo_cand* k, int S, int n_pad, int q, int K, QeiWork** out) {
    QeiWork* w = new QeiWork();
    memset(w, 0, sizeof(*w));
    w->m = k->m;
    w->S = S;
    w->n_pad = n_pad;
    w->q = q;
    w->K = K;
    int status = batch_alloc(ctx, k->m, k->m_pad, S, n_pad, q, &w->base);
    if (status != ROBO_OK) {
        delete w;
        return status;
    }
    BlockLayout lay(16);
    lay.add(&w->qs.z, (size_t)K * q);
    lay.add(&w->qs.b, (size_t)S * K);
    if (hipMalloc((void**)&w->d_block, lay.bytes()) != hipSuccess) {
        set_error("hipMalloc of %zu bytes failed (joint batch EI scenarios)", lay.bytes());
        batch_free(w->base);
        delete w;
        return ROBO_RUNTIME_ERROR;
    }
    lay.bind(w->d_block);
    w->qs.K = K;
    *out = w;
    return ROBO_OK;
}

void qei_free(QeiWork* w) {
    if (!w) return;
    batch_free(w->base);
    hipFree(w->d_block);
    hipFree(w->d_diag);
    delete w;
}

// the state is kept with gps[0] between calls of one (m, S, q, K)
static int qei_ensure(robo_gp* g, const robo_cand* k, int S, int q, int K, QeiWork** out) {
    QeiWork* w = g->qei;
    if (w && (w->m != k->m || w->S != S || w->n_pad < g->n_pad || w->q != q || w->K != K)) {
        ROBO_HIP_CHECK(hipStreamSynchronize(g->ctx->stream));
        qei_free(w);
        g->qei = w = nullptr;
    }
    if (!w) ROBO_TRY(qei_alloc(g->ctx, k, S, g->n_pad_max, q, K, &g->qei));
    *out = g->qei;
    return ROBO_OK;
}

static int launch_qei_scen(robo_gp* gp, const BatchState& st, const QeiState& qs, int s, int j, double b0) {
    hipLaunchKernelGGL(qei_scen_kernel, dim3(1), dim3(256), 0, gp->ctx->stream, st, qs, s, j, gp->y_std, b0);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

// one step of sample s for pick j >= 1: k_*(p_t) and d_t, beta_t, the scenarios, the conditioning pass, the fold
// events: EV_FOLD_BEGIN -> EV_FOLD_END around the fold kernel (the driver asks for the last pick's, last sample)
static int launch_qei_step(robo_gp* gp, const BatchState& st, const QeiState& qs, const robo_cand* cand, int s, int j,
                           bool events) {
    hipStream_t stream = gp->ctx->stream;
    const int n = gp->n, n_pad = gp->n_pad;
    const double* Xc = cand->d_Xc;
    const double* Xs = gp->d_Xs;
    const double* ism = gp->d_theta;
    double* w = st.w + (size_t)s * n_pad;
    double* v = st.v + (size_t)s * n_pad;
    hipLaunchKernelGGL(qei_kstar_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, stream, st, s, j, Xc, Xs, ism,
                       gp->cov, n, n_pad, 2.220446049250313e-16 / (gp->y_std * gp->y_std));
    ROBO_TRY(launch_fwd_rows(gp, w, v, st.stop));
    ROBO_TRY(launch_bwd_rows(gp, v, st.beta + (size_t)s * n_pad, st.stop));
    ROBO_TRY(launch_qei_scen(gp, st, qs, s, j, 0.0));
    const dim3 grid((unsigned)((st.m + BC_CAND - 1) / BC_CAND));
#define ROBO_QEI_COND_CALL(KIND)                                                                                          \
    do {                                                                                                                  \
        if (gp->dim <= 16)                                                                                                \
            hipLaunchKernelGGL((qei_cond_kernel<KIND, true>), grid, dim3(256), 0, stream, st, qs, s, j, Xc, Xs, ism, gp->cov, \
                               n, n_pad, gp->y_std);                                                                      \
        else                                                                                                              \
            hipLaunchKernelGGL((qei_cond_kernel<KIND, false>), grid, dim3(256), 0, stream, st, qs, s, j, Xc, Xs, ism, gp->cov, \
                               n, n_pad, gp->y_std);                                                                      \
    } while (0)
    if (gp->kind == ROBO_KERNEL_MATERN52_ARD) ROBO_QEI_COND_CALL(ROBO_KERNEL_MATERN52_ARD);
    else if (gp->kind == ROBO_KERNEL_RBF_ARD) ROBO_QEI_COND_CALL(ROBO_KERNEL_RBF_ARD);
    else ROBO_QEI_COND_CALL(ROBO_KERNEL_FABOLAS);
#undef ROBO_QEI_COND_CALL
    const size_t lds = ((size_t)64 * j + (size_t)4 * QF_ZK * j + qs.K + 256 + j) * sizeof(double);
    if (events) ROBO_TRY(record_phase(gp->ctx, EV_FOLD_BEGIN));
    hipLaunchKernelGGL(qei_fold_kernel, grid, dim3(256), lds, stream, st, qs, s, j, gp->y_std, cand->d_acq_sum);
    if (events) ROBO_TRY(record_phase(gp->ctx, EV_FOLD_END));
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

static void fill_nan(double* p, size_t from, size_t to) {
    for (size_t e = from; e < to; ++e) p[e] = std::nan("");
}

// marginal: pick 0 is robo_acq_eval_marginal_cand's sweep (accumulate, divide); otherwise robo_acq_eval_cand's
static int qei_core(robo_gp* const* gps, int32_t S, bool marginal, double par, const double* etas, robo_cand* k, int32_t q,
                    const double* z, int32_t K, int64_t* out_idx, double* out_gain, uint32_t* out_flags, int32_t* out_n_made,
                    double* out_acq, double* out_trace, double* out_coef, double* out_d, double* out_best) {
    if (!gps || S < 1 || !etas || !k || !out_idx) return ROBO_BAD_ARGUMENT;
    if (q < 1 || (int64_t)q > k->m || q > QEI_MAX_Q) {
        set_error("joint batch EI: q = %d outside 1 .. min(m = %lld, %d)", q, (long long)k->m, QEI_MAX_Q);
        return ROBO_BAD_ARGUMENT;
    }
    if (!z) {
        set_error("joint batch EI: the base samples z (K x q) are required");
        return ROBO_BAD_ARGUMENT;
    }
    if (K < 1 || K > QEI_MAX_K) {
        set_error("joint batch EI: K = %d scenarios outside 1 .. %d", K, QEI_MAX_K);
        return ROBO_BAD_ARGUMENT;
    }
    for (size_t e = 0; e < (size_t)K * q; ++e)
        if (!std::isfinite(z[e])) {
            set_error("joint batch EI: base sample z[%zu][%zu] is not finite", e / q, e % q);
            return ROBO_BAD_ARGUMENT;
        }
    for (int s = 0; s < S; ++s)
        if (gps[s] && !gps[s]->fitted) {
            set_error("joint batch EI: sample %d has no fitted model (Model has to be trained first!)", s);
            return ROBO_BAD_ARGUMENT;
        }
    const int verdict = ensemble_check("joint batch EI", ENSEMBLE_ONE_KIND_FP64, gps, S, k);
    if (verdict == ROBO_BAD_SHAPE || verdict == ROBO_NOT_FITTED) return ROBO_BAD_ARGUMENT;      // (its message stands)
    ROBO_TRY(verdict);
    robo_gp* g0 = gps[0];
    robo_ctx* c = g0->ctx;
    QeiWork* w = nullptr;
    ROBO_TRY(qei_ensure(g0, k, S, q, K, &w));
    BatchWork* bw = w->base;
    const size_t m = (size_t)k->m;
    const size_t trace_len = (size_t)q * S * m * 2;
    const size_t acq_len = out_acq ? (size_t)q * m : 0, coef_len = out_coef ? (size_t)(q - 1) * S * m : 0;
    const size_t best_len = out_best ? (size_t)q * S * K : 0;
    if (out_trace) ROBO_TRY(dev_grow(c->stream, &bw->d_trace, &bw->trace_cap, trace_len));
    ROBO_TRY(dev_grow(c->stream, &w->d_diag, &w->diag_cap, acq_len + coef_len + best_len));
    bw->st.q = q;
    bw->st.trace = out_trace ? bw->d_trace : nullptr;
    w->qs.acq = out_acq ? w->d_diag : nullptr;
    w->qs.coef = coef_len ? w->d_diag + acq_len : nullptr;
    w->qs.best = out_best ? w->d_diag + acq_len + coef_len : nullptr;
    const BatchState& st = bw->st;
    const QeiState& qs = w->qs;
    const bool state = q > 1 || out_trace || out_best;        // q = 1: the sweep alone

    // pick 0: the sweep, launch for launch, as batch.hip's batch_core
    ROBO_TRY(launch_batch_reset(c, st));
    if (q > 1) ROBO_TRY(upload_rows(c, "joint batch EI: upload of the base samples", {{w->qs.z, z, (size_t)K * q}}));
    for (int s = 0; s < S; ++s) {
        ROBO_TRY(clear_flags_on_error(k, predict_core(gps[s], k)));
        ROBO_TRY(clear_flags_on_error(k, launch_acq(c, k, ROBO_ACQ_EI, par, etas[s], marginal, s == 0)));
        if (state) {
            ROBO_TRY(clear_flags_on_error(k, launch_batch_init(gps[s], st, k, s, etas[s])));
            ROBO_TRY(clear_flags_on_error(k, launch_qei_scen(gps[s], st, qs, s, 0, etas[s] - par)));
        }
    }
    if (marginal) ROBO_TRY(clear_flags_on_error(k, launch_argmax(k, k->d_acq_sum, (double)S)));
    int status = launch_batch_record(c, st, k, 0, true);
    hipError_t e = hipSuccess;
    if (status == ROBO_OK && out_acq)
        e = hipMemcpyAsync(qs.acq, k->d_acq, m * sizeof(double), hipMemcpyDeviceToDevice, c->stream);
    // the later picks: launches only, ordered by the stream
    for (int j = 1; status == ROBO_OK && e == hipSuccess && j < q; ++j) {
        for (int s = 0; status == ROBO_OK && s < S; ++s)
            status = launch_qei_step(gps[s], st, qs, k, s, j, j == q - 1 && s == S - 1 && phase_events_on(c, k));
        if (status == ROBO_OK) status = launch_argmax(k, k->d_acq_sum, marginal ? (double)S : 1.0);
        if (status == ROBO_OK) status = launch_batch_record(c, st, k, j, false);
        if (status == ROBO_OK && out_acq)
            e = hipMemcpyAsync(qs.acq + (size_t)j * m, k->d_acq, m * sizeof(double), hipMemcpyDeviceToDevice, c->stream);
    }
    if (status == ROBO_OK && e != hipSuccess) {
        set_error("joint batch EI: copy of the values failed: %s", hipGetErrorString(e));
        status = ROBO_RUNTIME_ERROR;
    }
    // read-back: one copy of the report range into pinned memory (+ the diagnostics), the one synchronisation
    ROBO_TRY(finish_call(k, "joint batch EI", status, {{bw->h_report, bw->d_block + bw->rep_off, bw->rep_bytes},
                                                       {out_trace, bw->d_trace, trace_len * sizeof(double)},
                                                       {out_acq, qs.acq, acq_len * sizeof(double)},
                                                       {coef_len ? out_coef : nullptr, qs.coef, coef_len * sizeof(double)},
                                                       {out_best, qs.best, best_len * sizeof(double)}}));
    const double* hv = reinterpret_cast<const double*>(bw->h_report);
    const long long* hi = reinterpret_cast<const long long*>(bw->h_report + bw->off_idx);
    const unsigned* hf = reinterpret_cast<const unsigned*>(bw->h_report + bw->off_flg);
    for (int j = 0; j < q; ++j) {
        out_idx[j] = (int64_t)hi[j];
        if (out_gain) out_gain[j] = hv[j];
        if (out_flags) out_flags[j] = hf[j];
    }
    int made = 0;
    memcpy(&made, bw->h_report + bw->off_int, sizeof(int));
    if (out_n_made) *out_n_made = made;
    if (out_d) memcpy(out_d, bw->h_report + bw->off_fant, (size_t)q * S * sizeof(double));
    // the rows of the picks that were not made (a NaN winner ended the selection) say so
    const size_t done = (size_t)made;
    if (out_acq) fill_nan(out_acq, done * m, acq_len);
    if (out_trace) fill_nan(out_trace, done * S * m * 2, trace_len);
    if (coef_len) fill_nan(out_coef, (done > 0 ? done - 1 : 0) * S * m, coef_len);
    if (out_best) fill_nan(out_best, done * S * K, best_len);
    return ROBO_OK;
}

}  // namespace robo

using namespace robo;

extern "C" {

int32_t robo_qei_batch_cand(robo_gp* g, double par, double eta, robo_cand* k, int32_t q, const double* z, int32_t K,
                            int64_t* out_idx, double* out_gain, uint32_t* out_flags, int32_t* out_n_made, double* out_acq,
                            double* out_trace, double* out_coef, double* out_d, double* out_best) {
    return qei_core(&g, g ? 1 : 0, false, par, &eta, k, q, z, K, out_idx, out_gain, out_flags, out_n_made, out_acq, out_trace,
                    out_coef, out_d, out_best);
}

int32_t robo_qei_batch_marginal_cand(robo_gp* const* gps, int32_t S, double par, const double* etas, robo_cand* k, int32_t q,
                                     const double* z, int32_t K, int64_t* out_idx, double* out_gain, uint32_t* out_flags,
                                     int32_t* out_n_made, double* out_acq, double* out_trace, double* out_coef,
                                     double* out_d, double* out_best) {
    return qei_core(gps, S, true, par, etas, k, q, z, K, out_idx, out_gain, out_flags, out_n_made, out_acq, out_trace, out_coef,
                    out_d, out_best);
}

}  // extern "C"
