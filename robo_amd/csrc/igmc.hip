// Monte-Carlo entropy search (InformationGainMC), batched over candidates (DESIGN.md "Monte-Carlo entropy search").
//
// p_min of a belief N(m, V) over nb representer points by counting where each of nf draws  m + L z_f  has its minimum
// (robo/util/mc_part.py joint_pmin with given standard normals z), and the expected entropy change of that p_min when
// a candidate x is evaluated (the intended semantics of robo/acquisition_functions/information_gain_mc.py):
//   u   = v_x - sn2                                   (the reference's noise taken off a noise-free variance, sic)
//   a_b = (sqrt(v_x + 1e-10) / u) s_b                 s = cov(x, z_b)
//   V_x = Vb - s s^T / u,  L_x = chol(V_x + j I)      jitter ladder 0, 1e-9, x10 ... while j <= 1e4
//   value(b, p, f) = (Mb_b + a_b W_p) + (L_x z_f)_b   counted per outcome p: q_x[p][b] = max(count / nf, 1e-70)
//   gain = mean_p (H0 - H_p),  H_p = -sum_b q (log q + lmb_b)
// The same draws z serve the baseline p_min and every candidate (common random numbers).
//
//   igmc_kernel  one 256-thread workgroup per candidate (or per belief for the plain p_min: s = 0, one outcome W = 0):
//                V_x and its factor in LDS (row t in lane t, right-looking as ep.hip's ep_cholesky); then per tile of
//                256 draws each lane forms its draw's y = L z in registers (VALU fp64 FMAs over the lower triangle)
//                and, per outcome, the argmin over b (first index on ties, as np.argmin), counted with LDS integer
//                atomics into 16-bit halves of 32-bit words (order-independent); the entropies and their mean in a
//                fixed order by single lanes.  No workgroup reads another's results: a candidate's bits do not depend
//                on its batch position.
#include <cmath>
#include <vector>

#include "api_internal.h"

namespace robo {

constexpr int MC_MAX_NB = 64;
constexpr int MC_MAX_NP = 512;
constexpr int MC_MAX_NF = 65535;   // a count must fit 16 bits
constexpr int MC_LDA = 65;         // row stride of V / L in LDS: odd, so a column read by 64 lanes is conflict-free
constexpr int MC_PCH = 32;         // outcomes per LDS table of (Mb_b + a_b W_p)
constexpr double MC_DBL_MAX = 1.7976931348623157e308;

struct McArgs {
    int nb, np, nf;
    long long m;                    // workgroups = candidates or beliefs
    const double* mb;               // (nb) or (m, nb): mb_stride 0 or nb
    long long mb_stride;
    const double* vb;               // (nb, nb) or (m, nb, nb), row-major, lower triangle read
    long long vb_stride;
    const double* s;                // (m, lds) covariances with the representer points; nullptr: s = 0 (plain p_min)
    int lds;
    const double* var;              // (m) predictive variances (ignored when s is nullptr)
    double sn2;
    const double* w;                // (np) outcome quantiles
    const double* lmb;              // (nb) log proposal values (gain only)
    double h0;                      // entropy of the current p_min (gain only)
    const double* zt;               // (nb, ldz): draw f of row k at zt[k * ldz + f]
    int ldz;
    double* gain;                   // (m) or nullptr
    int* counts;                    // (m, np, nb) or nullptr
    double* jitter;                 // (m) or nullptr
    int* status;                    // (m) or nullptr: ROBO_OK / ROBO_NOT_POSITIVE_DEFINITE
    unsigned* flags;                // nullptr or a flag word: ROBO_FLAG_NOT_FACTORED is OR-ed in on a failed factor
};

// in-place lower Cholesky of the n x n matrix in sL, one lane per row; L_cc written on the diagonal.  LAPACK dpotrf's
// failure rule (a pivot that is not > 0, NaN included).  The result is uniform over the workgroup.
__device__ bool mc_cholesky(double* sL, int n) {
    const int t = threadIdx.x;
    for (int c = 0; c < n; ++c) {
        const double d = sL[c * MC_LDA + c];
        if (!(d > 0.0)) return false;
        const double ljj = sqrt(d);
        __syncthreads();            // every lane has read the pivot
        if (t == c) sL[c * MC_LDA + c] = ljj;
        if (t > c && t < n) sL[t * MC_LDA + c] = sL[t * MC_LDA + c] / ljj;
        __syncthreads();
        if (t > c && t < n) {
            const double lt = sL[t * MC_LDA + c];
            for (int j = c + 1; j <= t; ++j) sL[t * MC_LDA + j] = sL[t * MC_LDA + j] - lt * sL[j * MC_LDA + c];
        }
        __syncthreads();
    }
    return true;
}

// (Mb_b + a_b W_p) for outcomes p0 .. p0 + MC_PCH - 1 into sC[pp][b]; +inf for padded b (never a minimum)
template <int NBT>
__device__ void mc_outcome_table(double* sC, const double* smb, const double* sa, const double* w, int nb, int np,
                                 int p0) {
#pragma clang fp contract(off)
    for (int e = threadIdx.x; e < MC_PCH * NBT; e += 256) {
        const int pp = e / NBT, b = e - pp * NBT;
        double v = __builtin_huge_val();
        if (b < nb && p0 + pp < np) {
            const double dm = sa[b] * w[p0 + pp];
            v = smb[b] + dm;
        }
        sC[e] = v;
    }
}

// grid: m workgroups of 256; dynamic LDS: np * 32 words of packed 16-bit counters
template <int NBT>
__global__ __launch_bounds__(256) void igmc_kernel(McArgs A) {
#pragma clang fp contract(off)
    __shared__ double sL[MC_MAX_NB * MC_LDA];
    __shared__ double sC[MC_PCH * NBT];
    __shared__ double sH[MC_MAX_NP];
    __shared__ double smb[MC_MAX_NB], sa[MC_MAX_NB], ss[MC_MAX_NB];
    __shared__ double su;
    HIP_DYNAMIC_SHARED(unsigned, cnt)
    const int t = threadIdx.x, nb = A.nb, np = A.np, nf = A.nf;
    const long long c = blockIdx.x;
    const double* mb = A.mb + c * A.mb_stride;
    const double* vb = A.vb + c * A.vb_stride;

    // ---- innovation of the belief (information_gain.py:253-272 quirks: v - sn2, sqrt(v + 1e-10)) ----
    if (t == 0) su = A.s ? A.var[c] - A.sn2 : 1.0;
    __syncthreads();
    if (t < MC_MAX_NB) {
        double a = 0.0, sv = 0.0, m_ = 0.0;
        if (t < nb) {
            m_ = mb[t];
            if (A.s) {
                sv = A.s[c * A.lds + t];
                const double sc = sqrt(A.var[c] + 1e-10) / su;
                a = sc * sv;
            }
        }
        smb[t] = m_, sa[t] = a, ss[t] = sv;
    }
    __syncthreads();

    // ---- V_x + j I and its factor, the host's jitter ladder ----
    double jit = 0.0;
    bool ok = false;
    for (;;) {
        for (int e = t; e < MC_MAX_NB * MC_MAX_NB; e += 256) {
            const int r = e >> 6, q = e & 63;
            double v = 0.0;
            if (r < nb && q <= r) {
                v = vb[r * nb + q];
                if (A.s) {
                    const double ds = (ss[r] * ss[q]) / su;
                    v = v - ds;
                }
                if (r == q) v = v + jit;
            }
            sL[r * MC_LDA + q] = v;
        }
        __syncthreads();
        ok = mc_cholesky(sL, nb);
        if (ok) break;
        __syncthreads();            // every lane has left the factorisation before the next rebuild
        jit = jit == 0.0 ? 1e-9 : jit * 10.0;
        if (jit > 1e4) break;
    }
    if (!ok) {
        if (t == 0) {
            if (A.gain) A.gain[c] = -MC_DBL_MAX;
            if (A.jitter) A.jitter[c] = jit;
            if (A.status) A.status[c] = ROBO_NOT_POSITIVE_DEFINITE;
            if (A.flags) atomicOr(A.flags, ROBO_FLAG_NOT_FACTORED);
        }
        if (A.counts)
            for (int e = t; e < np * nb; e += 256) A.counts[c * np * nb + e] = 0;
        return;
    }

    // ---- count the argmins ----
    for (int e = t; e < np * 32; e += 256) cnt[e] = 0u;
    const int nch = (np + MC_PCH - 1) / MC_PCH;
    if (nch == 1) mc_outcome_table<NBT>(sC, smb, sa, A.w, nb, np, 0);
    __syncthreads();
    for (int f0 = 0; f0 < nf; f0 += 256) {
        const int f = f0 + t;
        const bool live = f < nf;
        double y[NBT];
#pragma unroll
        for (int b = 0; b < NBT; ++b) y[b] = 0.0;
#pragma unroll
        for (int k = 0; k < NBT; ++k) {
            if (k < nb) {                                   // uniform
                const double zk = live ? A.zt[(size_t)k * A.ldz + f] : 0.0;
#pragma unroll
                for (int b = k; b < NBT; ++b) y[b] = fma(sL[b * MC_LDA + k], zk, y[b]);
            }
        }
        for (int ch = 0; ch < nch; ++ch) {
            const int p0 = ch * MC_PCH;
            if (nch > 1) {
                __syncthreads();                            // every lane is done with the previous table
                mc_outcome_table<NBT>(sC, smb, sa, A.w, nb, np, p0);
                __syncthreads();
            }
            const int pn = np - p0 < MC_PCH ? np - p0 : MC_PCH;
            for (int pp = 0; pp < pn; ++pp) {
                const double* cp = sC + pp * NBT;
                double best = cp[0] + y[0];
                int idx = 0;
#pragma unroll
                for (int b = 1; b < NBT; ++b) {
                    const double v = cp[b] + y[b];
                    if (v < best) best = v, idx = b;
                }
                if (live) atomicAdd(&cnt[(p0 + pp) * 32 + (idx >> 1)], 1u << ((idx & 1) << 4));
            }
        }
    }
    __syncthreads();

    // ---- entropies, in b order per outcome, then their mean in p order ----
    const double dnf = (double)nf;
    for (int p = t; p < np; p += 256) {
        double acc = 0.0;
        for (int b = 0; b < nb; ++b) {
            const int n = (int)((cnt[p * 32 + (b >> 1)] >> ((b & 1) << 4)) & 0xFFFFu);
            if (A.counts) A.counts[(c * np + p) * nb + b] = n;
            if (A.gain) {
                double q = (double)n / dnf;
                q = q < 1e-70 ? 1e-70 : q;
                const double lq = log(q) + A.lmb[b];
                acc = acc + q * lq;
            }
        }
        sH[p] = -acc;
    }
    __syncthreads();
    if (t == 0) {
        if (A.gain) {
            double acc = 0.0;
            for (int p = 0; p < np; ++p) acc = acc + (A.h0 - sH[p]);
            double g = acc / (double)np;
            if (!isfinite(g)) g = -MC_DBL_MAX;                // information_gain.py:119-120
            A.gain[c] = g;
        }
        if (A.jitter) A.jitter[c] = jit;
        if (A.status) A.status[c] = ROBO_OK;
    }
}

static int launch_igmc(robo_ctx* ctx, const McArgs& a) {
    if (a.m < 1) return ROBO_OK;
    const size_t shm = (size_t)a.np * 32 * sizeof(unsigned);
    const dim3 grid((unsigned)a.m), block(256);
    if (a.nb <= 16) hipLaunchKernelGGL(igmc_kernel<16>, grid, block, shm, ctx->stream, a);
    else if (a.nb <= 32) hipLaunchKernelGGL(igmc_kernel<32>, grid, block, shm, ctx->stream, a);
    else if (a.nb <= 48) hipLaunchKernelGGL(igmc_kernel<48>, grid, block, shm, ctx->stream, a);
    else hipLaunchKernelGGL(igmc_kernel<64>, grid, block, shm, ctx->stream, a);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

// ---- device buffers: one grow-once set per context; the draws are uploaded only when they change ----
struct McWork {
    double *d_zt, *d_mb, *d_vb, *d_w, *d_lmb, *d_s, *d_v, *d_gain, *d_jit;
    int *d_counts, *d_status;
    size_t cap_zt, cap_mb, cap_vb, cap_w, cap_lmb, cap_s, cap_v, cap_gain, cap_jit, cap_counts, cap_status;
    std::vector<double> zkey;       // the draws d_zt holds: (nb, nf, z...)
};

void mc_release(robo_ctx* c) {
    McWork* w = c->mc;
    if (!w) return;
    for (double* p : {w->d_zt, w->d_mb, w->d_vb, w->d_w, w->d_lmb, w->d_s, w->d_v, w->d_gain, w->d_jit}) hipFree(p);
    hipFree(w->d_counts);
    hipFree(w->d_status);
    delete w;
    c->mc = nullptr;
}

static McWork* mc_work(robo_ctx* c) {
    if (!c->mc) c->mc = new McWork();
    return c->mc;
}

static int mc_check(int nb, int np, int nf) {
    if (nb < 1 || nb > MC_MAX_NB || np < 1 || np > MC_MAX_NP || nf < 1 || nf > MC_MAX_NF) {
        set_error("Monte-Carlo p_min: nb=%d must be in [1, %d], n_outcomes=%d in [1, %d], nf=%d in [1, %d]", nb,
                  MC_MAX_NB, np, MC_MAX_NP, nf, MC_MAX_NF);
        return ROBO_BAD_ARGUMENT;
    }
    return ROBO_OK;
}

// z (nf, nb) host, row-major -> d_zt (nb, nf), skipped when the same draws are already there
static int mc_upload_z(robo_ctx* c, int nb, int nf, const double* z) {
    McWork* w = mc_work(c);
    const size_t n = (size_t)nb * nf;
    if (w->zkey.size() == n + 2 && w->zkey[0] == (double)nb && w->zkey[1] == (double)nf && w->d_zt &&
        memcmp(w->zkey.data() + 2, z, n * sizeof(double)) == 0)
        return ROBO_OK;
    w->zkey.clear();
    ROBO_TRY(dev_grow(c->stream, &w->d_zt, &w->cap_zt, n));
    std::vector<double> zt(n);
    for (int f = 0; f < nf; ++f)
        for (int k = 0; k < nb; ++k) zt[(size_t)k * nf + f] = z[(size_t)f * nb + k];
    ROBO_HIP_CHECK(hipMemcpyAsync(w->d_zt, zt.data(), n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));   // the staging vector dies with this scope
    w->zkey.resize(n + 2);
    w->zkey[0] = (double)nb, w->zkey[1] = (double)nf;
    memcpy(w->zkey.data() + 2, z, n * sizeof(double));
    return ROBO_OK;
}

static int mc_upload(robo_ctx* c, double** d, size_t* cap, const double* h, size_t n) {
    ROBO_TRY(dev_grow(c->stream, d, cap, n));
    ROBO_HIP_CHECK(hipMemcpyAsync(*d, h, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return ROBO_OK;
}

// the gains of m candidates whose s (m, lds) and v (m) are on the device, into d_gain (asynchronous); counts / jitter:
// device buffers or nullptr
int mc_eval_gains(robo_ctx* c, int64_t m, int nb, int np, int nf, double sn2, const double* d_s, int lds,
                  const double* d_v, const double* Mb, const double* Vb, const double* logP, const double* lmb,
                  const double* W, const double* z, double* d_gain, int* d_counts, double* d_jit, unsigned* d_flags) {
    ROBO_TRY(mc_check(nb, np, nf));
    if (!Mb || !Vb || !logP || !lmb || !W || !z) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(mc_upload_z(c, nb, nf, z));
    McWork* w = c->mc;
    ROBO_TRY(mc_upload(c, &w->d_mb, &w->cap_mb, Mb, (size_t)nb));
    ROBO_TRY(mc_upload(c, &w->d_vb, &w->cap_vb, Vb, (size_t)nb * nb));
    ROBO_TRY(mc_upload(c, &w->d_w, &w->cap_w, W, (size_t)np));
    ROBO_TRY(mc_upload(c, &w->d_lmb, &w->cap_lmb, lmb, (size_t)nb));
    double h0 = 0.0;                                   // -sum_b p_b (log p_b + lmb_b), p = exp(logP), in b order
    for (int b = 0; b < nb; ++b) h0 = h0 - std::exp(logP[b]) * (logP[b] + lmb[b]);
    McArgs a;
    memset(&a, 0, sizeof(a));
    a.nb = nb, a.np = np, a.nf = nf, a.m = m;
    a.mb = w->d_mb, a.vb = w->d_vb;
    a.s = d_s, a.lds = lds, a.var = d_v, a.sn2 = sn2;
    a.w = w->d_w, a.lmb = w->d_lmb, a.h0 = h0;
    a.zt = w->d_zt, a.ldz = nf;
    a.gain = d_gain, a.counts = d_counts, a.jitter = d_jit, a.flags = d_flags;
    return launch_igmc(c, a);
}

}  // namespace robo

using namespace robo;

extern "C" int32_t robo_pmin_mc(robo_ctx* ctx, int32_t S, int32_t nb, int32_t nf, const double* mu, const double* sigma,
                                const double* z, double* out_pmin, double* out_jitter, int32_t* out_status) {
    if (!ctx || S < 1 || !mu || !sigma || !z || !out_pmin || !out_status) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(mc_check(nb, 1, nf));
    ROBO_HIP_CHECK(hipSetDevice(ctx->device));
    ROBO_TRY(mc_upload_z(ctx, nb, nf, z));
    McWork* w = ctx->mc;
    hipStream_t st = ctx->stream;
    const size_t n1 = (size_t)S * nb;
    const double zero = 0.0;
    ROBO_TRY(mc_upload(ctx, &w->d_mb, &w->cap_mb, mu, n1));
    ROBO_TRY(mc_upload(ctx, &w->d_vb, &w->cap_vb, sigma, n1 * nb));
    ROBO_TRY(mc_upload(ctx, &w->d_w, &w->cap_w, &zero, 1));
    ROBO_TRY(dev_grow(ctx->stream, &w->d_counts, &w->cap_counts, n1));
    ROBO_TRY(dev_grow(ctx->stream, &w->d_jit, &w->cap_jit, (size_t)S));
    ROBO_TRY(dev_grow(ctx->stream, &w->d_status, &w->cap_status, (size_t)S));
    McArgs a;
    memset(&a, 0, sizeof(a));
    a.nb = nb, a.np = 1, a.nf = nf, a.m = S;
    a.mb = w->d_mb, a.mb_stride = nb, a.vb = w->d_vb, a.vb_stride = (long long)nb * nb;
    a.w = w->d_w, a.zt = w->d_zt, a.ldz = nf;
    a.counts = w->d_counts, a.jitter = w->d_jit, a.status = w->d_status;
    ROBO_TRY(launch_igmc(ctx, a));
    std::vector<int> counts(n1);
    std::vector<double> jit((size_t)S);
    ROBO_HIP_CHECK(hipMemcpyAsync(counts.data(), w->d_counts, n1 * sizeof(int), hipMemcpyDeviceToHost, st));
    ROBO_HIP_CHECK(hipMemcpyAsync(jit.data(), w->d_jit, (size_t)S * sizeof(double), hipMemcpyDeviceToHost, st));
    ROBO_HIP_CHECK(hipMemcpyAsync(out_status, w->d_status, (size_t)S * sizeof(int), hipMemcpyDeviceToHost, st));
    ROBO_HIP_CHECK(hipStreamSynchronize(st));
    for (size_t i = 0; i < n1; ++i) {                  // np.maximum(wins / Nf, 1e-70)
        const double p = (double)counts[i] / (double)nf;
        out_pmin[i] = p < 1e-70 ? 1e-70 : p;
    }
    if (out_jitter) memcpy(out_jitter, jit.data(), (size_t)S * sizeof(double));
    return ROBO_OK;
}

extern "C" int32_t robo_igmc_eval_moments(robo_ctx* ctx, int64_t m, int32_t nb, int32_t n_outcomes, int32_t nf,
                                          double sn2, const double* s, const double* v, const double* Mb,
                                          const double* Vb, const double* logP, const double* lmb, const double* W,
                                          const double* z, double* out_dh, int32_t* out_counts, double* out_jitter) {
    if (!ctx || m < 1 || !s || !v || !out_dh) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(mc_check(nb, n_outcomes, nf));
    ROBO_HIP_CHECK(hipSetDevice(ctx->device));
    McWork* w = mc_work(ctx);
    hipStream_t st = ctx->stream;
    const size_t nc = out_counts ? (size_t)m * n_outcomes * nb : 0;
    ROBO_TRY(mc_upload(ctx, &w->d_s, &w->cap_s, s, (size_t)m * nb));
    ROBO_TRY(mc_upload(ctx, &w->d_v, &w->cap_v, v, (size_t)m));
    ROBO_TRY(dev_grow(ctx->stream, &w->d_gain, &w->cap_gain, (size_t)m));
    if (out_counts) ROBO_TRY(dev_grow(ctx->stream, &w->d_counts, &w->cap_counts, nc));
    if (out_jitter) ROBO_TRY(dev_grow(ctx->stream, &w->d_jit, &w->cap_jit, (size_t)m));
    ROBO_TRY(mc_eval_gains(ctx, m, nb, n_outcomes, nf, sn2, w->d_s, nb, w->d_v, Mb, Vb, logP, lmb, W, z, w->d_gain,
                           out_counts ? w->d_counts : nullptr, out_jitter ? w->d_jit : nullptr, nullptr));
    ROBO_HIP_CHECK(hipMemcpyAsync(out_dh, w->d_gain, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
    if (out_counts)
        ROBO_HIP_CHECK(hipMemcpyAsync(out_counts, w->d_counts, nc * sizeof(int), hipMemcpyDeviceToHost, st));
    if (out_jitter)
        ROBO_HIP_CHECK(hipMemcpyAsync(out_jitter, w->d_jit, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
    ROBO_HIP_CHECK(hipStreamSynchronize(st));
    return ROBO_OK;
}
