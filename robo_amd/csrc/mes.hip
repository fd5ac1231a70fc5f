// Max-value entropy search (Wang & Jegelka, ICML 2017) for minimisation, resident on the device (robo_mes_eval_cand,
// robo_mes_eval_marginal_cand, robo_mes_sample_min_moments, robo_mes_eval_moments; no counterpart in the reference).
//
//   sweep (predict.hip, unchanged) -> mes_bracket_kernel + mes_bracket_final_kernel: w_lo, w_hi
//   -> up to MES_PASSES x [ mes_f_kernel: F at the 63 interior points of the three quantiles' brackets, per 128 candidates
//                           -> mes_section_kernel: partials added in block order, every bracket cut to one section ]
//   -> mes_gumbel_kernel: w_1/4, w_1/2, w_3/4, (a, b), y*_k
//   -> mes_value_kernel: alpha_i = (1/K) sum_k [ gamma phi(gamma) / (2 Phi(gamma)) - log Phi(gamma) ]
//   -> the sweep's own reduction (launch_argmax, acq.hip)
//
// The rule (include/robo_hip.h): sigma_i = sqrt(v_i), F(w) = sum_i log Phi((w + mu_i) / sigma_i) is the log-probability
// that max_i(-f_i) < w for independent f_i; [w_lo, w_hi] = [max_i(-mu_i - 8 sigma_i), max_i(-mu_i + 8 sigma_i)] brackets
// every quantile above Phi(-8) and below Phi(8)^M, so no bracket search is needed.
//
// Ordering is the stream's alone: brackets, quantiles, Gumbel parameters and y* stay in device memory between the
// kernels, a pass that finds every bracket narrow enough raises `done` and the remaining passes return at once.
// Every sum has a fixed order: a workgroup of the F pass adds ITS 128 candidates in index order per grid point, the
// section kernel adds the workgroups' partials in block order; no floating-point atomics.
#include "api_internal.h"
#include "kern_math.h"

namespace robo {
constexpr const char* MES_LABEL = "max-value entropy search";
constexpr int MES_G = 64;                       // sections per pass and quantile
constexpr int MES_PTS = 3 * (MES_G - 1);        // interior grid points of the three brackets: 189
constexpr int MES_F_THREADS = 192;              // one grid point per work-item (3 idle)
constexpr int MES_CHUNK = 128;                  // candidates per workgroup of the F pass: fixes the order of every sum
constexpr int MES_PASSES = 10;                  // 2^-60 of the first bracket; the end condition needs 2^-46 (8 - 9 passes)
constexpr int MES_MAX_K = 128;
constexpr double MES_GUMBEL_DEN = -1.5725335836855194;      // log log(4/3) - log log 4
constexpr double MES_LOGLOG2 = -0.36651292058166435;        // log log 2
constexpr double MES_CONVERGED = 0.0, MES_OPEN = 1.0, MES_NAN_MOMENT = 2.0;   // MesState::status

__device__ __forceinline__ double mes_nan() { return __longlong_as_double(0x7FF8000000000000LL); }
__device__ __forceinline__ double mes_ninf() { return -__builtin_huge_val(); }
// log 1/4, log 1/2, log 3/4
__device__ __forceinline__ double mes_log_p(int q) {
    return q == 0 ? -1.3862943611198906 : (q == 1 ? -0.6931471805599453 : -0.2876820724517809);
}

// grid point j of the bracket [a, b] (j = 0 and MES_G are a and b themselves and are never formed here); one fused
// operation, so that the F pass and the section kernel agree on every bit
__device__ __forceinline__ double mes_grid_point(double a, double b, int j) { return fma(b - a, (double)j * (1.0 / MES_G), a); }

// one candidate's term of F(w); sigma == 0 is a step at w = -mu
__device__ __forceinline__ double mes_f_term(double w, double mu, double sigma) {
    if (sigma == 0.0) return w < -mu ? mes_ninf() : 0.0;
    return norm_logcdf((w + mu) / sigma);
}

// one draw's term of alpha; 0 * inf from a huge gamma counts as 0.  For gamma << 0 the two parts are each ~gamma^2 / 2 and
// cancel to ~log(-gamma): the relative error grows like gamma^2 eps (range stated in include/robo_hip.h)
__device__ __forceinline__ double mes_value_term(double gamma) {
    const double lc = norm_logcdf(gamma);
    const double r = exp(norm_logpdf(gamma) - lc);          // phi / Phi; exp(x < -745) = 0
    const double t = r == 0.0 ? 0.0 : gamma * r * 0.5;
    return t - lc;
}

// per MES_CHUNK candidates: max(-mu - 8 sigma), max(-mu + 8 sigma), "some moment is NaN"; optionally the moments
// themselves into the trace (m x 2)
__global__ __launch_bounds__(MES_CHUNK) void mes_bracket_kernel(MesState st, const double* __restrict__ mean,
                                                                const double* __restrict__ var,
                                                                double* __restrict__ trace) {
    __shared__ double sh[3][MES_CHUNK / 64];
    const long long i = (long long)blockIdx.x * MES_CHUNK + threadIdx.x;
    double lo = mes_ninf(), hi = mes_ninf(), bad = 0.0;
    if (i < st.m) {
        const double mu = mean[i], v = var[i];
        const double sigma = sqrt(v);
        if (trace) {
            trace[i * 2] = mu;
            trace[i * 2 + 1] = v;
        }
        if (isnan(mu) || isnan(sigma)) {
            bad = 1.0;
        } else {
            lo = -mu - 8.0 * sigma;
            hi = -mu + 8.0 * sigma;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        lo = fmax(lo, __shfl_xor(lo, o));
        hi = fmax(hi, __shfl_xor(hi, o));
        bad = fmax(bad, __shfl_xor(bad, o));
    }
    if ((threadIdx.x & 63) == 0) {
        sh[0][threadIdx.x >> 6] = lo;
        sh[1][threadIdx.x >> 6] = hi;
        sh[2][threadIdx.x >> 6] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* p = st.bpart + (size_t)blockIdx.x * 3;
        p[0] = fmax(sh[0][0], sh[0][1]);
        p[1] = fmax(sh[1][0], sh[1][1]);
        p[2] = fmax(sh[2][0], sh[2][1]);
    }
}

// single workgroup: the maxima over the partials (exact in any order) -> gumbel[0..1], the three brackets, `done`
__global__ __launch_bounds__(256) void mes_bracket_final_kernel(MesState st, int s) {
    __shared__ double sh[3][4];
    double lo = mes_ninf(), hi = mes_ninf(), bad = 0.0;
    for (int p = threadIdx.x; p < st.nblk; p += 256) {
        lo = fmax(lo, st.bpart[(size_t)p * 3]);
        hi = fmax(hi, st.bpart[(size_t)p * 3 + 1]);
        bad = fmax(bad, st.bpart[(size_t)p * 3 + 2]);
    }
    for (int o = 32; o > 0; o >>= 1) {
        lo = fmax(lo, __shfl_xor(lo, o));
        hi = fmax(hi, __shfl_xor(hi, o));
        bad = fmax(bad, __shfl_xor(bad, o));
    }
    if ((threadIdx.x & 63) == 0) {
        sh[0][threadIdx.x >> 6] = lo;
        sh[1][threadIdx.x >> 6] = hi;
        sh[2][threadIdx.x >> 6] = bad;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 4; ++w) {
        lo = fmax(lo, sh[0][w]);
        hi = fmax(hi, sh[1][w]);
        bad = fmax(bad, sh[2][w]);
    }
    double* g = st.gumbel + (size_t)s * 7;
    if (bad != 0.0) {
        for (int e = 0; e < 7; ++e) g[e] = mes_nan();
        st.status[s] = MES_NAN_MOMENT;
        *st.done = 1;
        return;
    }
    g[0] = lo;
    g[1] = hi;
    for (int q = 0; q < 3; ++q) {
        st.brk[q] = lo;
        st.brk[3 + q] = hi;
    }
    st.brk[6] = (hi - lo) * 1.4210854715202004e-14;     // 2^-46 of the first bracket
    st.status[s] = MES_OPEN;
    *st.done = 0;
}

// F at every interior grid point of the three brackets over this workgroup's MES_CHUNK candidates, each loaded once
__global__ __launch_bounds__(MES_F_THREADS) void mes_f_kernel(MesState st, const double* __restrict__ mean,
                                                              const double* __restrict__ var) {
    __shared__ double sMu[MES_CHUNK], sSig[MES_CHUNK];
    if (*st.done) return;
    const int t = threadIdx.x;
    const long long base = (long long)blockIdx.x * MES_CHUNK;
    const int cnt = st.m - base < MES_CHUNK ? (int)(st.m - base) : MES_CHUNK;
    if (t < cnt) {
        sMu[t] = mean[base + t];
        sSig[t] = sqrt(var[base + t]);
    }
    __syncthreads();
    if (t >= MES_PTS) return;
    const int q = t / (MES_G - 1), j = t - q * (MES_G - 1) + 1;
    const double w = mes_grid_point(st.brk[q], st.brk[3 + q], j);
    double sum = 0.0;
    for (int c = 0; c < cnt; ++c) sum += mes_f_term(w, sMu[c], sSig[c]);
    st.fpart[(size_t)blockIdx.x * MES_F_THREADS + t] = sum;
}

// single workgroup: F = the partials in block order; per quantile the first grid point with F >= log p closes the new
// bracket.  All three no wider than max(2^-46 of the first bracket, 4 ulp): done.
__global__ __launch_bounds__(MES_F_THREADS) void mes_section_kernel(MesState st, int s) {
    __shared__ double sF[MES_F_THREADS];
    __shared__ int sOk[3];
    if (*st.done) return;
    const int t = threadIdx.x;
    double sum = 0.0;
    if (t < MES_PTS)
        for (int p = 0; p < st.nblk; ++p) sum += st.fpart[(size_t)p * MES_F_THREADS + t];
    sF[t] = sum;
    __syncthreads();
    if (t < 3) {
        const double a = st.brk[t], b = st.brk[3 + t], logp = mes_log_p(t);
        const double* f = sF + t * (MES_G - 1);
        int k = MES_G;
        for (int j = MES_G - 1; j >= 1; --j)
            if (f[j - 1] >= logp) k = j;
        const double na = k == 1 ? a : mes_grid_point(a, b, k - 1);
        const double nb = k == MES_G ? b : mes_grid_point(a, b, k);
        st.brk[t] = na;
        st.brk[3 + t] = nb;
        const double big = fmax(fabs(na), fabs(nb));
        const double ulp = __longlong_as_double(__double_as_longlong(big) + 1) - big;
        sOk[t] = nb - na <= fmax(st.brk[6], 4.0 * ulp);
    }
    __syncthreads();
    if (t == 0 && sOk[0] && sOk[1] && sOk[2]) {
        st.status[s] = MES_CONVERGED;
        *st.done = 1;
    }
}

// the quantiles (bracket midpoints), the Gumbel fit and the K draws of sample s.  (a, b) are formed with single,
// never contracted operations: they equal the same expressions evaluated on the host bit for bit.
__global__ __launch_bounds__(MES_MAX_K) void mes_gumbel_kernel(MesState st, int s, int clamp, double eta) {
    __shared__ double sAB[2];
    double* g = st.gumbel + (size_t)s * 7;
    const bool ok = st.status[s] != MES_NAN_MOMENT;
    if (threadIdx.x == 0 && ok) {
        const double w25 = 0.5 * (st.brk[0] + st.brk[3]), w50 = 0.5 * (st.brk[1] + st.brk[4]);
        const double w75 = 0.5 * (st.brk[2] + st.brk[5]);
        const double b = rn_div(rn_sub(w25, w75), MES_GUMBEL_DEN);
        const double a = rn_add(w50, rn_mul(b, MES_LOGLOG2));
        g[2] = w25;
        g[3] = w50;
        g[4] = w75;
        g[5] = a;
        g[6] = b;
        sAB[0] = a;
        sAB[1] = b;
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k >= st.K) return;
    double y = mes_nan();
    if (ok) {
        y = -rn_sub(sAB[0], rn_mul(sAB[1], log(-log(st.u[(size_t)s * st.K + k]))));
        if (clamp && y > eta) y = eta;
    }
    st.ystar[(size_t)s * st.K + k] = y;
}

// mode 1: sum[i] = alpha   (the only or first hyper-parameter sample)
// mode 2: sum[i] += alpha  (next samples; fixed sample order, as acq_kernel)
__global__ __launch_bounds__(256) void mes_value_kernel(const double* __restrict__ mean, const double* __restrict__ var,
                                                        long long m, const double* __restrict__ ystar, int K, int mode,
                                                        double* __restrict__ acq_sum, unsigned* __restrict__ flags) {
    __shared__ double sY[MES_MAX_K];
    if (threadIdx.x < K) sY[threadIdx.x] = ystar[threadIdx.x];
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const double mu = mean[i], v = var[i];
    const double sigma = sqrt(v);
    unsigned f = 0;
    double a;
    if (isnan(mu) || isnan(sigma)) {
        a = mes_nan();
    } else if (sigma == 0.0) {
        a = 0.0;
        f |= ROBO_FLAG_ZERO_SIGMA;
    } else {
        double sum = 0.0;
        for (int k = 0; k < K; ++k) sum += mes_value_term((mu - sY[k]) / sigma);
        a = sum / (double)K;
    }
    if (isnan(a)) f |= ROBO_FLAG_NAN;
    if (f != 0) atomicOr(flags, f);
    if (mode == 1) acq_sum[i] = a;
    else acq_sum[i] += a;
}

// ---- host side ------------------------------------------------------------------------------------------------------------
int mes_alloc(int64_t m, int S, int K, MesWork** out) {
    MesWork* w = new MesWork();
    w->m = m;
    w->S = S;
    w->K = K;
    MesState& st = w->st;
    const int nblk = (int)((m + MES_CHUNK - 1) / MES_CHUNK);
    // [ystar | gumbel | status] is what a call reports: ONE copy into pinned memory, so one entry
    w->rep_doubles = (size_t)S * K + (size_t)S * 7 + (size_t)S;
    BlockLayout lay(sizeof(double));
    lay.add(&st.ystar, w->rep_doubles);
    lay.add(&st.u, (size_t)S * K);
    lay.add(&st.brk, 8);
    lay.add(&st.bpart, (size_t)nblk * 3);
    lay.add(&st.fpart, (size_t)nblk * MES_F_THREADS);
    lay.add(&st.done, 1);
    if (hipMalloc((void**)&w->d_block, lay.bytes()) != hipSuccess) {
        set_error("hipMalloc of %zu bytes failed (max-value entropy search state)", lay.bytes());
        delete w;
        return ROBO_RUNTIME_ERROR;
    }
    if (hipHostMalloc((void**)&w->h_stage, (w->rep_doubles + (size_t)S * K) * sizeof(double)) != hipSuccess) {
        set_error("hipHostMalloc failed (max-value entropy search report)");
        hipFree(w->d_block);
        delete w;
        return ROBO_RUNTIME_ERROR;
    }
    lay.bind(w->d_block);
    st.gumbel = st.ystar + (size_t)S * K;
    st.status = st.gumbel + (size_t)S * 7;
    st.m = m;
    st.K = K;
    st.nblk = nblk;
    *out = w;
    return ROBO_OK;
}

void mes_free(MesWork* w) {
    if (!w) return;
    hipFree(w->d_block);
    hipFree(w->d_trace);
    if (w->h_stage) hipHostFree(w->h_stage);
    delete w;
}

static int mes_check_draws(const double* u, int64_t count, int K) {
    if (K < 1 || K > MES_MAX_K) {
        set_error("max-value entropy search: K = %d outside 1 .. %d", K, MES_MAX_K);
        return ROBO_BAD_ARGUMENT;
    }
    for (int64_t e = 0; e < count; ++e)
        if (!(u[e] > 0.0 && u[e] < 1.0)) {
            set_error("max-value entropy search: u[%lld] = %g is not inside the open interval (0, 1)", (long long)e, u[e]);
            return ROBO_BAD_ARGUMENT;
        }
    return ROBO_OK;
}

// u (S x K, host) -> the state block, through the pinned stage behind the report
static int mes_upload_draws(robo_ctx* c, MesWork* w, const double* u) {
    double* hu = w->h_stage + w->rep_doubles;
    const size_t n = (size_t)w->S * w->K;
    memcpy(hu, u, n * sizeof(double));
    ROBO_HIP_CHECK(hipMemcpyAsync(w->st.u, hu, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return ROBO_OK;
}

// bracket, quantile search, Gumbel fit and draws of sample s from the moments in d_mean / d_var (asynchronous)
static int launch_mes_sample(robo_ctx* c, const MesState& st, int s, const double* d_mean, const double* d_var,
                             double* d_trace, int clamp, double eta) {
    hipStream_t stream = c->stream;
    hipLaunchKernelGGL(mes_bracket_kernel, dim3((unsigned)st.nblk), dim3(MES_CHUNK), 0, stream, st, d_mean, d_var, d_trace);
    hipLaunchKernelGGL(mes_bracket_final_kernel, dim3(1), dim3(256), 0, stream, st, s);
    for (int p = 0; p < MES_PASSES; ++p) {
        hipLaunchKernelGGL(mes_f_kernel, dim3((unsigned)st.nblk), dim3(MES_F_THREADS), 0, stream, st, d_mean, d_var);
        hipLaunchKernelGGL(mes_section_kernel, dim3(1), dim3(MES_F_THREADS), 0, stream, st, s);
    }
    hipLaunchKernelGGL(mes_gumbel_kernel, dim3(1), dim3(MES_MAX_K), 0, stream, st, s, clamp, eta);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

static int launch_mes_value(robo_cand* k, const double* d_ystar, int K, bool first) {
    hipLaunchKernelGGL(mes_value_kernel, dim3((unsigned)((k->m + 255) / 256)), dim3(256), 0, k->ctx->stream,
                       (const double*)k->d_mean, (const double*)k->d_var, (long long)k->m, d_ystar, K, first ? 1 : 2,
                       k->d_acq_sum, k->d_flags);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

// the report of a finished call (after its synchronisation): status of every sample, then the diagnostics
static int mes_take_report(const MesWork* w, double* out_ystar, double* out_gumbel) {
    const size_t nk = (size_t)w->S * w->K;
    const double* status = w->h_stage + nk + (size_t)w->S * 7;
    for (int s = 0; s < w->S; ++s) {
        if (status[s] == MES_NAN_MOMENT) {
            set_error("max-value entropy search: a mean or variance of sample %d is NaN (or a variance negative)", s);
            return ROBO_BAD_ARGUMENT;
        }
        if (status[s] != MES_CONVERGED) {
            set_error("max-value entropy search: the quantile search of sample %d did not reach its end condition", s);
            return ROBO_RUNTIME_ERROR;
        }
    }
    if (out_ystar) memcpy(out_ystar, w->h_stage, nk * sizeof(double));
    if (out_gumbel) memcpy(out_gumbel, w->h_stage + nk, (size_t)w->S * 7 * sizeof(double));
    return ROBO_OK;
}

static int mes_ensure(robo_gp* g, const robo_cand* k, int S, int K, MesWork** out) {
    MesWork* w = g->mes;
    if (w && (w->m != k->m || w->S != S || w->K != K)) {
        ROBO_HIP_CHECK(hipStreamSynchronize(g->ctx->stream));
        mes_free(w);
        g->mes = w = nullptr;
    }
    if (!w) ROBO_TRY(mes_alloc(k->m, S, K, &g->mes));
    *out = g->mes;
    return ROBO_OK;
}

static int mes_core(robo_gp* const* gps, int32_t S, const double* etas, robo_cand* k, const double* u, int32_t K,
                    int32_t clamp, double* out_acq, double* out_max, int64_t* out_argmax, uint32_t* out_flags,
                    double* out_ystar, double* out_gumbel, double* out_trace) {
    if (!gps || S < 1 || !etas || !k || !u) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(mes_check_draws(u, (int64_t)S * (K > 0 ? K : 0), K));
    ROBO_TRY(ensemble_check(MES_LABEL, ENSEMBLE_MES_VERDICTS, gps, S, k));
    robo_gp* g0 = gps[0];
    robo_ctx* c = g0->ctx;
    MesWork* w = nullptr;
    ROBO_TRY(mes_ensure(g0, k, S, K, &w));
    const size_t trace_len = (size_t)S * k->m * 2;
    if (out_trace) ROBO_TRY(dev_grow(c->stream, &w->d_trace, &w->trace_cap, trace_len));
    const MesState& st = w->st;
    ROBO_TRY(mes_upload_draws(c, w, u));
    // event slots 27 -> 30 -> 31 bracket the tail of the LAST sample: minimum sampling, element-wise half
    const bool ev = phase_events_on(c, k);
    for (int s = 0; s < S; ++s) {
        ROBO_TRY(clear_flags_on_error(k, predict_core(gps[s], k)));
        ROBO_TRY(clear_flags_on_error(k, launch_mes_sample(c, st, s, k->d_mean, k->d_var,
                                                      out_trace ? w->d_trace + (size_t)s * k->m * 2 : nullptr, clamp, etas[s])));
        if (ev) ROBO_TRY(record_phase(c, EV_FOLD_BEGIN));
        ROBO_TRY(clear_flags_on_error(k, launch_mes_value(k, st.ystar + (size_t)s * K, K, s == 0)));
        if (ev) ROBO_TRY(record_phase(c, EV_FOLD_END));
    }
    ROBO_TRY(clear_flags_on_error(k, launch_argmax(k, k->d_acq_sum, (double)S)));
    ROBO_TRY(finish_call(k, MES_LABEL, ROBO_OK, {{w->h_stage, w->d_block, w->rep_doubles * sizeof(double)},
                                                 {out_trace, w->d_trace, trace_len * sizeof(double)}}, false));
    // (max, argmax, flags) [+ the values] and the one synchronisation of the call
    ROBO_TRY(clear_flags_on_error(k, acq_read_back(k, k->d_acq, out_acq, out_max, out_argmax, out_flags)));
    return mes_take_report(w, out_ystar, out_gumbel);
}

}  // namespace robo

using namespace robo;

extern "C" {

int32_t robo_mes_eval_cand(robo_gp* g, double eta, robo_cand* k, const double* u, int32_t K, int32_t clamp, double* out_acq,
                           double* out_max, int64_t* out_argmax, uint32_t* out_flags, double* out_ystar,
                           double* out_gumbel, double* out_trace) {
    return mes_core(&g, g ? 1 : 0, &eta, k, u, K, clamp, out_acq, out_max, out_argmax, out_flags, out_ystar, out_gumbel,
                    out_trace);
}

int32_t robo_mes_eval_marginal_cand(robo_gp* const* gps, int32_t S, const double* etas, robo_cand* k, const double* u,
                                    int32_t K, int32_t clamp, double* out_acq, double* out_max, int64_t* out_argmax,
                                    uint32_t* out_flags, double* out_ystar, double* out_gumbel, double* out_trace) {
    return mes_core(gps, S, etas, k, u, K, clamp, out_acq, out_max, out_argmax, out_flags, out_ystar, out_gumbel, out_trace);
}

int32_t robo_mes_sample_min_moments(robo_ctx* ctx, const double* mean, const double* var, int64_t m, const double* u,
                                    int32_t K, int32_t clamp, double eta, double* out_ystar, double* out_gumbel) {
    if (!ctx || !mean || !var || !u) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(mes_check_draws(u, K > 0 ? K : 0, K));
    robo_cand* k = nullptr;
    ROBO_TRY(moments_handle(ctx, mean, var, m, "max-value entropy search: upload of the moments", &k));
    MesWork* w = nullptr;
    int st = mes_alloc(m, 1, K, &w);
    if (st == ROBO_OK) st = mes_upload_draws(ctx, w, u);
    if (st == ROBO_OK) st = launch_mes_sample(ctx, w->st, 0, k->d_mean, k->d_var, nullptr, clamp, eta);
    if (w) st = finish_call(k, MES_LABEL, st, {{w->h_stage, w->d_block, w->rep_doubles * sizeof(double)}});
    if (st == ROBO_OK) st = mes_take_report(w, out_ystar, out_gumbel);
    mes_free(w);
    robo_cand_destroy(k);
    return st;
}

int32_t robo_mes_eval_moments(robo_ctx* ctx, const double* mean, const double* var, int64_t m, const double* ystar,
                              int32_t K, double* out_acq, double* out_max, int64_t* out_argmax, uint32_t* out_flags) {
    if (!ctx || !mean || !var || !ystar) return ROBO_BAD_ARGUMENT;
    if (K < 1 || K > MES_MAX_K) {
        set_error("max-value entropy search: K = %d outside 1 .. %d", K, MES_MAX_K);
        return ROBO_BAD_ARGUMENT;
    }
    robo_cand* k = nullptr;
    ROBO_TRY(moments_handle(ctx, mean, var, m, "max-value entropy search: upload of the moments", &k));
    // y* (K <= 128 <= m_pad doubles) rides in the handle's d_q, which the moments form never fills: no state block, no
    // pinned allocation -- this entry point runs once per point under the single-point maximisers
    int st = upload_rows(ctx, "max-value entropy search: upload of y*", {{k->d_q, ystar, (size_t)K}});
    if (st == ROBO_OK) st = launch_mes_value(k, k->d_q, K, true);
    return moments_finish(k, st, true, out_acq, out_max, out_argmax, out_flags);
}

}  // extern "C"
