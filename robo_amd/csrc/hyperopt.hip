// Multi-start MAP optimisation of the GP hyper-parameters, resident on the device.
//
// Replaces the host loop of GaussianProcess.optimize (robo/models/gaussian_process.py:193-219: SciPy's L-BFGS-B on nll with
// finite-difference gradients, P + 1 fits and synchronisations per gradient, one start, a 1e25 wall outside the prior's
// support) for the priors the library evaluates itself.  The objective is
//     F(theta) = log p(y | X, theta) + log prior(theta),
// invalid (the reference's protocol) when any |theta_p| > 20, the factorisation fails or the prior is not finite.  All
// starts advance in lock step, one batched evaluation of (F, G) per iteration, nothing read back in between:
//   hyper_propose_kernel  per start: L-BFGS two-loop direction from its last pairs (s, y), projection onto the box, the trial
//                         z = clip(x + alpha d); then the batch fit's FitSample, 1 / sqrt(metric) and the inputs scaled by the
//                         trial's metrics (mcmc_propose_scale_kernel's job)
//   gram / potrf          the batched fit of gram.hip / potrf.hip with the inverse diagonal blocks
//   gradient.hip          launch_grad_loglik_batch: W = L^-1, A = alpha alpha^T - K^-1, the reductions, S samples per launch
//   hyper_accept_kernel   F and G (chain rule on the noise entry, analytic prior gradient), the Armijo test, the pair update,
//                         step length, status and the trace record
// Every sum runs in a fixed order (block_dot), so two calls return the same bits.  Frozen and dead starts keep a harmless
// sample in the batch (their own point / the unit kernel); their results are not looked at.
#include <cmath>
#include <vector>

#include "api_internal.h"
#include "mcmc_dev.h"

namespace robo {

constexpr double HYPER_ALPHA_MIN = 9.094947017729282e-13;   // 2^-40
constexpr double HYPER_PAIR_TOL = 1e-10;
enum { HYPER_LIVE = 0, HYPER_CONVERGED = 1, HYPER_STALLED = 2, HYPER_DEAD = 3 };
// what the propose kernel leaves for the accept kernel: no trial (frozen or dead), a trial, a trial made after dropping the
// pairs, no direction left
enum { PEND_NONE = 0, PEND_TRIAL = 1, PEND_TRIAL_DROPPED = 2, PEND_NO_DIRECTION = 3 };

// sum_p a[p] b[p] over p < P in a fixed order: thread t adds p = t, t + 256, ..., a butterfly per wave, the four waves in
// order.  Contains barriers: every thread of the block calls it.  sred: 4 doubles of LDS.
__device__ __forceinline__ double block_dot(const double* a, const double* b, int P, double* sred) {
    double s = 0.0;
    for (int p = threadIdx.x; p < P; p += 256) s += a[p] * b[p];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    __syncthreads();   // sred free
    if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = s;
    __syncthreads();
    return (sred[0] + sred[1]) + (sred[2] + sred[3]);
}

// largest |g_p| over the components that do not point out of the box at a bound of x
__device__ __forceinline__ double block_projected_max(const double* x, const double* g, const double* lower,
                                                      const double* upper, int P, double* sred) {
    double m = 0.0;
    for (int p = threadIdx.x; p < P; p += 256) {
        const double gp = g[p];
        const bool out = (x[p] <= lower[p] && gp < 0.0) || (x[p] >= upper[p] && gp > 0.0);
        const double a = out ? 0.0 : fabs(gp);
        m = (a > m || a != a) ? a : m;       // a NaN component is not "converged"
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double v = __shfl_xor(m, o);
        m = (v > m || v != v) ? v : m;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = m;
    __syncthreads();
    double r = sred[0];
    for (int w = 1; w < 4; ++w) r = (sred[w] > r || sred[w] != sred[w]) ? sred[w] : r;
    return r;
}

__device__ __forceinline__ double clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }   // NaN stays

// d log prior / d theta_p of the priors of mcmc_dev.h (prior_lnprob), where the prior is finite
__device__ __forceinline__ double prior_grad(int kind, const double* th, int p, int P, const double* par) {
    if (kind == 0) return 0.0;
    if (p == 0) {              // lognormal on theta_0 - loc
        const double v = th[0] - par[0];
        return -(log(v) / (par[1] * par[1]) + 1.0) / v;
    }
    if (p == P - 1) {          // horseshoe on the noise
        const double s2 = par[4] * par[4], e2 = exp(2.0 * th[p]);
        return -6.0 * s2 / ((3.0 * s2 + e2) * log(1.0 + 3.0 * s2 / e2));
    }
    if (kind == 2) {           // EnvPrior: NormalPrior.lnprob is a pdf
        const int ls_end = 1 + (int)par[5], lr_end = ls_end + (int)par[6];
        if (p >= ls_end && p < lr_end) {
            const double u = (th[p] - par[7]) / par[8];
            const double pdf = exp(-0.5 * (u * u)) / (par[8] * sqrt(2.0 * M_PI));
            return -(u / par[8]) * pdf;
        }
    }
    return 0.0;                // tophat
}

// grid (blocks over the rows of X, starts): EVERY block forms its start's trial point in LDS, then scales its share of X;
// block 0 of each start leaves the trial, its step length, the verdict for the accept kernel and the FitSample behind.  No
// block writes anything another block of this launch reads.
__global__ __launch_bounds__(256) void hyper_propose_kernel(HyperState st, int t, const double* __restrict__ X,
                                                            double* __restrict__ Xs, long long rows_real, long long rows_pad,
                                                            size_t xs_stride) {
    __shared__ double sz[MAX_DIM + 8];      // the trial point
    __shared__ double sd[MAX_DIM + 8];      // the direction
    __shared__ double sism[MAX_DIM];
    __shared__ double sa[HYPER_MAX_HISTORY], ssy[HYPER_MAX_HISTORY];
    __shared__ double sred[4];
    __shared__ int sbad;
    const int k = blockIdx.y, P = st.P, D = st.D, tid = threadIdx.x;
    const double* x = st.x + (size_t)k * P;
    const double* g = st.g + (size_t)k * P;
    const int state = t == 0 ? HYPER_LIVE : st.state[k];
    int pend = PEND_NONE;
    double alpha = t == 0 ? st.step0 : st.alpha[k];
    if (tid == 0) sbad = 0;
    if (t == 0) {
        for (int p = tid; p < P; p += 256) sz[p] = clip(x[p], st.lower[p], st.upper[p]);
        pend = PEND_TRIAL;
    } else if (state != HYPER_LIVE) {
        for (int p = tid; p < P; p += 256) sz[p] = x[p];
    } else {
        const int m = st.npairs[k];
        const double* S = st.sh + (size_t)k * st.hist * P;
        const double* Y = st.yh + (size_t)k * st.hist * P;
        for (int p = tid; p < P; p += 256) sd[p] = g[p];
        if (m == 0) {
            const double nrm = sqrt(block_dot(g, g, P, sred));
            for (int p = tid; p < P; p += 256) sd[p] = nrm > 0.0 ? g[p] / nrm : 0.0;
        } else {
            for (int i = m - 1; i >= 0; --i) {
                const double sy = block_dot(S + (size_t)i * P, Y + (size_t)i * P, P, sred);
                const double a = block_dot(S + (size_t)i * P, sd, P, sred) / sy;
                if (tid == 0) {
                    ssy[i] = sy;
                    sa[i] = a;
                }
                for (int p = tid; p < P; p += 256) sd[p] -= a * Y[(size_t)i * P + p];
            }
            __syncthreads();       // ssy / sa
            const double gamma = ssy[m - 1] / block_dot(Y + (size_t)(m - 1) * P, Y + (size_t)(m - 1) * P, P, sred);
            for (int p = tid; p < P; p += 256) sd[p] *= gamma;
            for (int i = 0; i < m; ++i) {
                const double b = block_dot(Y + (size_t)i * P, sd, P, sred) / ssy[i];
                for (int p = tid; p < P; p += 256) sd[p] += (sa[i] - b) * S[(size_t)i * P + p];
            }
        }
        // projection: no component leaves the box at a bound
        for (int p = tid; p < P; p += 256)
            if ((x[p] <= st.lower[p] && sd[p] < 0.0) || (x[p] >= st.upper[p] && sd[p] > 0.0)) sd[p] = 0.0;
        pend = PEND_TRIAL;
        const double dg = block_dot(sd, g, P, sred);
        if (!(dg > 0.0)) {         // not an ascent direction: drop the pairs, projected steepest ascent
            for (int p = tid; p < P; p += 256)
                sd[p] = ((x[p] <= st.lower[p] && g[p] < 0.0) || (x[p] >= st.upper[p] && g[p] > 0.0)) ? 0.0 : g[p];
            const double nrm = sqrt(block_dot(sd, sd, P, sred));
            if (nrm > 0.0) {
                for (int p = tid; p < P; p += 256) sd[p] /= nrm;
                pend = PEND_TRIAL_DROPPED;
            } else {
                pend = PEND_NO_DIRECTION;
            }
        }
        for (int p = tid; p < P; p += 256)
            sz[p] = pend == PEND_NO_DIRECTION ? x[p] : clip(x[p] + alpha * sd[p], st.lower[p], st.upper[p]);
    }
    __syncthreads();               // sz, sbad = 0
    bool bad = false;
    for (int p = tid; p < P; p += 256) bad = bad || !(sz[p] >= -20.0 && sz[p] <= 20.0);   // also true for NaN / inf
    if (bad) sbad = 1;
    __syncthreads();
    const bool ok = sbad == 0;     // outside the reference's bounds: the unit kernel keeps the slot harmless
    const bool fab = st.kind == ROBO_KERNEL_FABOLAS;
    const int n_metric = fab ? D - 1 : D;
    for (int d = tid; d < D; d += 256) sism[d] = d < n_metric ? exp(-0.5 * (ok ? sz[1 + d] : 0.0)) : 1.0;
    __syncthreads();
    if (blockIdx.x == 0) {
        for (int p = tid; p < P; p += 256) st.z[(size_t)k * P + p] = sz[p];
        for (int d = tid; d < D; d += 256) st.d_ism[(size_t)k * D + d] = sism[d];
        if (tid == 0) {
            st.aused[k] = alpha;
            st.pending[k] = pend;
            FitSample sp;
            sp.cov.kind = st.kind;
            sp.cov.dim = D;
            sp.cov.amp = exp(ok ? sz[0] : 0.0);
            sp.cov.blr_a = fab ? exp(ok ? sz[D] : 0.0) : 0.0;
            sp.cov.blr_b = fab ? exp(ok ? sz[D + 1] : 0.0) : 0.0;
            sp.noise = exp(ok ? sz[P - 1] : 0.0) + JITTER;
            sp.mean_c = st.mean_c;
            sp.direct = gram_needs_direct(st.kind, sism, st.d_x2max, D);
            st.d_sp[k] = sp;
        }
    }
    // scale_inputs_kernel's arithmetic: pad rows replicate row 0
    double* out = Xs + (size_t)k * xs_stride;
    const long long total = rows_pad * D;
    for (long long i = (long long)blockIdx.x * blockDim.x + tid; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / D;
        const int d = (int)(i - r * D);
        const long long src = r < rows_real ? r : 0;
        out[i] = rows_real > 0 ? X[src * D + d] * sism[d] : 0.0;
    }
}

// one workgroup per start: F and G at the trial, the accept test and everything that follows from it
__global__ __launch_bounds__(256) void hyper_accept_kernel(HyperState st, int t) {
    __shared__ double sz[MAX_DIM + 8];      // the trial point
    __shared__ double sG[MAX_DIM + 8];      // its gradient
    __shared__ double ss[MAX_DIM + 8];      // z - x
    __shared__ double sy[MAX_DIM + 8];      // g - G(z)
    __shared__ double sred[4];
    __shared__ double sF;
    __shared__ int sbad, svalid;
    const int k = blockIdx.x, P = st.P, tid = threadIdx.x;
    const double nan = __builtin_nan(""), ninf = -__builtin_huge_val();
    double* x = st.x + (size_t)k * P;
    double* g = st.g + (size_t)k * P;
    const double* z = st.z + (size_t)k * P;
    double* tr = st.trace ? st.trace + ((size_t)t * st.K + k) * (2 * P + 3) : nullptr;
    const int pend = st.pending[k];
    if (pend == PEND_NONE || pend == PEND_NO_DIRECTION) {
        // frozen earlier, dead, or frozen now for want of a direction: the entry repeats the start's point
        if (tr) {
            for (int p = tid; p < P; p += 256) {
                tr[p] = x[p];
                tr[P + 1 + p] = g[p];
            }
            if (tid == 0) {
                tr[P] = st.f[k];
                tr[2 * P + 1] = st.alpha[k];
                tr[2 * P + 2] = 2.0;
            }
        }
        if (tid == 0 && pend == PEND_NO_DIRECTION) {
            st.state[k] = HYPER_STALLED;
            st.npairs[k] = 0;
        }
        return;
    }
    if (tid == 0) sbad = 0;
    for (int p = tid; p < P; p += 256) sz[p] = z[p];
    __syncthreads();
    bool bad = false;
    for (int p = tid; p < P; p += 256) bad = bad || !(sz[p] >= -20.0 && sz[p] <= 20.0);
    if (bad) sbad = 1;
    __syncthreads();
    if (tid == 0) {
        const int fail = st.d_fail[k];
        if (fail < 0) atomicOr(st.err, 1);   // a panel follower's hand-off timed out (potrf.hip): not a property of theta
        const double ll = -0.5 * (st.d_out[2 * k] + st.d_out[2 * k + 1] + (double)st.n * log(2.0 * M_PI));
        double prior = 0.0;
        bool valid = sbad == 0 && fail == 0;
        if (valid && st.prior_kind != 0) prior = prior_lnprob(st.prior_kind, sz, P, st.prior_par);
        const double F = ll + prior;
        valid = valid && prior > ninf && prior < __builtin_huge_val() && F > ninf && F < __builtin_huge_val();
        sF = valid ? F : ninf;
        svalid = valid ? 1 : 0;
    }
    __syncthreads();
    const bool valid = svalid != 0;
    const double F = sF;
    for (int p = tid; p < P; p += 256) {
        double G = nan;
        if (valid) {
            G = st.d_grad[(size_t)k * P + p];
            if (p == P - 1) G *= exp(sz[p]);       // d / d log sigma^2 = sigma^2 d / d sigma^2
            G += prior_grad(st.prior_kind, sz, p, P, st.prior_par);
        }
        sG[p] = G;
        ss[p] = sz[p] - x[p];
        sy[p] = g[p] - G;
    }
    const double aused = st.aused[k];
    int code;
    if (t == 0) {
        code = valid ? 1 : 3;
        const double pm = valid ? block_projected_max(sz, sG, st.lower, st.upper, P, sred) : 0.0;
        for (int p = tid; p < P; p += 256) {
            x[p] = sz[p];
            g[p] = sG[p];
        }
        if (tid == 0) {
            st.f[k] = valid ? F : nan;
            st.alpha[k] = st.step0;
            st.npairs[k] = 0;
            st.state[k] = !valid ? HYPER_DEAD : (pm <= st.gtol ? HYPER_CONVERGED : HYPER_LIVE);
        }
    } else {
        int m = pend == PEND_TRIAL_DROPPED ? 0 : st.npairs[k];
        const double f = st.f[k];
        const double sg = block_dot(ss, g, P, sred);
        const bool accept = valid && F >= f + st.c1 * sg;
        code = accept ? 1 : (valid ? 0 : 3);
        if (accept) {
            const double s_y = block_dot(ss, sy, P, sred), s_s = block_dot(ss, ss, P, sred), y_y = block_dot(sy, sy, P, sred);
            if (s_y > HYPER_PAIR_TOL * (sqrt(s_s) * sqrt(y_y))) {
                double* S = st.sh + (size_t)k * st.hist * P;
                double* Y = st.yh + (size_t)k * st.hist * P;
                if (m == st.hist) {        // the oldest pair drops (every thread moves its own columns)
                    for (int p = tid; p < P; p += 256)
                        for (int i = 0; i + 1 < m; ++i) {
                            S[(size_t)i * P + p] = S[(size_t)(i + 1) * P + p];
                            Y[(size_t)i * P + p] = Y[(size_t)(i + 1) * P + p];
                        }
                    m -= 1;
                }
                for (int p = tid; p < P; p += 256) {
                    S[(size_t)m * P + p] = ss[p];
                    Y[(size_t)m * P + p] = sy[p];
                }
                m += 1;
            }
            const double pm = block_projected_max(sz, sG, st.lower, st.upper, P, sred);
            for (int p = tid; p < P; p += 256) {
                x[p] = sz[p];
                g[p] = sG[p];
            }
            if (tid == 0) {
                st.f[k] = F;
                st.alpha[k] = 1.0;
                if (pm <= st.gtol) st.state[k] = HYPER_CONVERGED;
            }
        } else if (tid == 0) {
            const double a = aused / 2.0;
            st.alpha[k] = a;
            if (a < HYPER_ALPHA_MIN) st.state[k] = HYPER_STALLED;
        }
        if (tid == 0) st.npairs[k] = m;
    }
    if (tr) {
        for (int p = tid; p < P; p += 256) {
            tr[p] = sz[p];
            tr[P + 1 + p] = sG[p];
        }
        if (tid == 0) {
            tr[P] = F;
            tr[2 * P + 1] = aused;
            tr[2 * P + 2] = (double)code;
        }
    }
}

// the start with the largest final F (the first of equals; dead starts never win) -> out = [theta | F | index]
__global__ __launch_bounds__(64) void hyper_result_kernel(HyperState st) {
    __shared__ int sbest;
    if (threadIdx.x == 0) {
        int best = -1;
        for (int k = 0; k < st.K; ++k)
            if (st.state[k] != HYPER_DEAD && (best < 0 || st.f[k] > st.f[best])) best = k;
        sbest = best;
        st.out[st.P] = best < 0 ? __builtin_nan("") : st.f[best];
        st.out[st.P + 1] = (double)best;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < st.P; p += 64) st.out[p] = sbest < 0 ? __builtin_nan("") : st.x[(size_t)sbest * st.P + p];
}

int launch_hyper_propose(robo_ctx* ctx, const HyperState& st, int t, const double* d_X, double* d_Xs, int64_t rows_real,
                         int64_t rows_pad, size_t xs_stride) {
    int blocks = (int)((rows_pad * st.D + 255) / 256);
    if (blocks > 64) blocks = 64;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(hyper_propose_kernel, dim3(blocks, st.K), dim3(256), 0, ctx->stream, st, t, d_X, d_Xs,
                       (long long)rows_real, (long long)rows_pad, xs_stride);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_hyper_accept(robo_ctx* ctx, const HyperState& st, int t) {
    hipLaunchKernelGGL(hyper_accept_kernel, dim3(st.K), dim3(256), 0, ctx->stream, st, t);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_hyper_result(robo_ctx* ctx, const HyperState& st) {
    hipLaunchKernelGGL(hyper_result_kernel, dim3(1), dim3(64), 0, ctx->stream, st);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

void hyper_free(HyperWork* w) {
    if (!w) return;
    hipFree(w->d_V);
    hipFree(w->d_A);
    hipFree(w->d_alpha);
    hipFree(w->d_part);
    hipFree(w->d_out);
    hipFree(w->d_block);
    hipFree(w->d_trace);
    delete w;
}

static size_t tiles64(const robo_gp* g) {
    const size_t t64 = ((size_t)g->n + 63) / 64;
    return t64 * (t64 + 1) / 2;
}

// bytes one sample takes in the batch workspace of the fit and in the gradient workspace behind it
static size_t hyper_sample_bytes(const robo_gp* g) {
    const size_t np = (size_t)g->n_pad, D = (size_t)g->dim, P = (size_t)robo_theta_size(g->kind, g->dim);
    return (3 * np * np + np * (NB + D) + np + P * tiles64(g) + P) * sizeof(double);
}

// the gradient workspace for `cap` samples at the current n_pad: allocated here, before any launch
static int hyper_grad_ensure(robo_gp* g, int cap) {
    if (!g->hyper) g->hyper = new HyperWork();
    HyperWork* w = g->hyper;
    const int P = robo_theta_size(g->kind, g->dim);
    if (w->g_cap >= cap && w->g_npad == g->n_pad && w->g_P == P) return ROBO_OK;
    hipFree(w->d_V); hipFree(w->d_A); hipFree(w->d_alpha); hipFree(w->d_part); hipFree(w->d_out);
    w->d_V = w->d_A = w->d_alpha = w->d_part = w->d_out = nullptr;
    w->g_cap = 0;
    const size_t np = (size_t)g->n_pad, n = (size_t)cap;
    // the reduction's 64-row tiles are counted for n_pad rows: the workspace also serves a later, larger n of this n_pad
    const size_t t64 = np / 64, nt = t64 * (t64 + 1) / 2;
    ROBO_TRY(dev_alloc(&w->d_V, n * np * np));
    ROBO_TRY(dev_alloc(&w->d_A, n * np * np));
    ROBO_TRY(dev_alloc(&w->d_alpha, n * np));
    ROBO_TRY(dev_alloc(&w->d_part, n * (size_t)P * nt));
    ROBO_TRY(dev_alloc(&w->d_out, n * (size_t)P));
    w->g_cap = cap;
    w->g_npad = g->n_pad;
    w->g_P = P;
    return ROBO_OK;
}

static FitBuffers batch_buffers(robo_gp* g, int ns, double* host_out) {
    const size_t np = (size_t)g->n_pad;
    FitBuffers fb;
    fb.K = g->d_bK; fb.k_stride = np * np;
    fb.prog = g->d_bprog;
    fb.Linv = g->d_bLinv; fb.linv_stride = np * NB;
    fb.Xs = g->d_bXs; fb.xs_stride = np * (size_t)g->dim;
    fb.sp = g->d_bsp;
    fb.fail = g->d_bfail;
    fb.out = g->d_bout;
    fb.ll_part = g->d_bllpart;
    fb.LinvP = nullptr;
    fb.host_out = host_out;
    fb.want_inverse = true;            // the gradient starts from the inverse diagonal blocks
    fb.skip_tail = false;
    fb.S = ns;
    return fb;
}

static GradBatch grad_buffers(robo_gp* g, int ns) {
    const size_t np = (size_t)g->n_pad;
    const HyperWork* w = g->hyper;
    GradBatch gb;
    gb.K = g->d_bK; gb.k_stride = np * np;
    gb.Linv = g->d_bLinv; gb.linv_stride = np * NB;
    gb.Xs = g->d_bXs; gb.xs_stride = np * (size_t)g->dim;
    gb.sp = g->d_bsp;
    gb.V = w->d_V; gb.A = w->d_A;
    gb.alpha = w->d_alpha; gb.part = w->d_part; gb.out = w->d_out;
    gb.S = ns;
    return gb;
}

}  // namespace robo

using namespace robo;

extern "C" {

int32_t robo_gp_grad_loglik_batch(robo_gp* g, const double* thetas, int32_t S, double mean_c, double* out_loglik,
                                  double* out_grad, int32_t* out_status) {
    if (!g || !thetas || S < 0 || !out_loglik || !out_grad) return ROBO_BAD_ARGUMENT;
    if (!g->has_data) {
        set_error("robo_gp_grad_loglik_batch before robo_gp_set_data");
        return ROBO_NOT_FITTED;
    }
    if (S == 0) return ROBO_OK;
    robo_ctx* c = g->ctx;
    const int P = robo_theta_size(g->kind, g->dim), D = g->dim;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    int chunk = (int)(workspace_bytes(c) / hyper_sample_bytes(g));
    if (chunk < 1) {
        set_error("robo_gp_grad_loglik_batch: one sample of n_pad %d (%zu bytes) exceeds the workspace (ws_bytes)", g->n_pad,
                  hyper_sample_bytes(g));
        return ROBO_BAD_SHAPE;
    }
    if (chunk > S) chunk = S;
    g->fitted = false;
    ROBO_TRY(batch_ensure(g, chunk));
    ROBO_TRY(hyper_grad_ensure(g, chunk));
    const double nan = std::nan("");
    for (int s0 = 0; s0 < S; s0 += chunk) {
        const int ns = S - s0 < chunk ? S - s0 : chunk;
        const int cap = g->b_cap;                          // layout of the staging block and of its device twin
        FitSample* hsp = reinterpret_cast<FitSample*>(g->h_bstage);
        double* hism = reinterpret_cast<double*>(hsp + cap);
        double* hout = hism + (size_t)cap * D;             // [ns][5]: z.z, log det, failure flag, min / max L_ii
        std::vector<int> status(ns, ROBO_OK);
        bool any_direct = false;
        for (int s = 0; s < ns; ++s) {
            status[s] = theta_to_sample(g, thetas + (size_t)(s0 + s) * P, mean_c, hsp + s, hism + (size_t)s * D);
            if (status[s] != ROBO_OK) {   // keep the slot numerically harmless: unit kernel
                static const double zeros[MAX_DIM + 8] = {0};
                theta_to_sample(g, zeros, mean_c, hsp + s, hism + (size_t)s * D);
            }
            if (hsp[s].direct) any_direct = true;
        }
        ROBO_HIP_CHECK(hipMemcpyAsync(g->d_bsp, hsp, (size_t)cap * sizeof(FitSample) + (size_t)ns * D * sizeof(double),
                                      hipMemcpyHostToDevice, c->stream));
        const size_t np = (size_t)g->n_pad;
        ROBO_TRY(launch_scale_inputs(c, g->d_X, g->d_bXs, g->d_bism, g->n, g->n_pad, D, ns, np * D, (size_t)D));
        FitBuffers fb = batch_buffers(g, ns, hout);
        fb.gram_mixed = any_direct;
        ROBO_TRY(launch_potrf(g, fb, true));
        ROBO_TRY(launch_grad_loglik_batch(g, grad_buffers(g, ns)));
        ROBO_HIP_CHECK(hipMemcpyAsync(out_grad + (size_t)s0 * P, g->hyper->d_out, (size_t)ns * P * sizeof(double),
                                      hipMemcpyDeviceToHost, c->stream));
        ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));   // the one synchronisation of a group; hout is pinned
        for (int s = 0; s < ns; ++s) {
            double ll = -HUGE_VAL;
            if (status[s] == ROBO_OK) {
                if (hout[5 * s + 2] < 0.0) status[s] = ROBO_RUNTIME_ERROR;      // a follower's hand-off timed out (potrf.hip)
                else if (hout[5 * s + 2] != 0.0) status[s] = ROBO_NOT_POSITIVE_DEFINITE;
                else ll = -0.5 * (hout[5 * s] + hout[5 * s + 1] + (double)g->n * std::log(2.0 * M_PI));
            }
            out_loglik[s0 + s] = ll;
            if (status[s] != ROBO_OK)
                for (int p = 0; p < P; ++p) out_grad[(size_t)(s0 + s) * P + p] = nan;
            if (out_status) out_status[s0 + s] = status[s];
        }
    }
    return ROBO_OK;
}

int32_t robo_gp_optimize_hypers(robo_gp* g, double mean_c, int32_t prior_kind, const double* prior_par, const double* lower,
                                const double* upper, const double* starts, int32_t n_starts, int32_t n_iters, int32_t history,
                                double step0, double c1, double gtol, double* out_theta, double* out_value, int32_t* out_best,
                                double* out_final, double* out_values, int32_t* out_status, double* out_trace) {
    if (!g || !lower || !upper || !starts || !out_theta || !out_value || !out_best) return ROBO_BAD_ARGUMENT;
    if (n_starts < 1 || n_starts > HYPER_MAX_STARTS || history < 1 || history > HYPER_MAX_HISTORY || n_iters < 0) {
        set_error("robo_gp_optimize_hypers: n_starts=%d (1 .. %d), history=%d (1 .. %d), n_iters=%d (>= 0)", n_starts,
                  HYPER_MAX_STARTS, history, HYPER_MAX_HISTORY, n_iters);
        return ROBO_BAD_ARGUMENT;
    }
    if (!(step0 > 0.0) || !(c1 >= 0.0) || !(gtol >= 0.0)) {
        set_error("robo_gp_optimize_hypers: step0=%g c1=%g gtol=%g", step0, c1, gtol);
        return ROBO_BAD_ARGUMENT;
    }
    const int D = g->dim, P = robo_theta_size(g->kind, D);
    if (prior_kind != 0 && ((prior_kind != 1 && prior_kind != 2) || !prior_par)) {
        set_error("robo_gp_optimize_hypers: prior kind %d (0 = none, 1 = DefaultPrior, 2 = EnvPrior)", prior_kind);
        return ROBO_BAD_ARGUMENT;
    }
    if (prior_kind == 2) {
        const double n_ls = prior_par[5], n_lr = prior_par[6];
        if (!(n_ls >= 0 && n_lr >= 0 && n_ls == (double)(int)n_ls && n_lr == (double)(int)n_lr &&
              1 + (int)n_ls + (int)n_lr <= P - 1) || !(prior_par[8] > 0.0)) {
            set_error("robo_gp_optimize_hypers: EnvPrior with n_ls=%g n_lr=%g sigma=%g does not fit %d hyper-parameters", n_ls,
                      n_lr, prior_par[8], P);
            return ROBO_BAD_ARGUMENT;
        }
    }
    for (int p = 0; p < P; ++p)
        if (!(lower[p] <= upper[p])) {
            set_error("robo_gp_optimize_hypers: lower[%d]=%g > upper[%d]=%g", p, lower[p], p, upper[p]);
            return ROBO_BAD_ARGUMENT;
        }
    if (!g->has_data) {
        set_error("robo_gp_optimize_hypers before robo_gp_set_data");
        return ROBO_NOT_FITTED;
    }
    robo_ctx* c = g->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    const int K = n_starts;
    const size_t np = (size_t)g->n_pad;
    if ((size_t)K * hyper_sample_bytes(g) > workspace_bytes(c)) {   // all starts advance in one batched pass
        set_error("robo_gp_optimize_hypers: %d starts of n_pad %zu exceed the workspace (ws_bytes)", K, np);
        return ROBO_BAD_SHAPE;
    }
    g->fitted = false;
    ROBO_TRY(batch_ensure(g, K));
    ROBO_TRY(hyper_grad_ensure(g, K));
    HyperWork* w = g->hyper;
    // one state block: doubles first, then ints
    const size_t KP = (size_t)K * P, pairs = KP * (size_t)history, n_int = 3 * (size_t)K + 1;
    HyperState st;
    memset(&st, 0, sizeof(st));
    BlockLayout lay(sizeof(double));
    lay.add(&st.lower, (size_t)P);
    lay.add(&st.upper, (size_t)P);
    lay.add(&st.x, KP);
    lay.add(&st.g, KP);
    lay.add(&st.z, KP);
    lay.add(&st.f, (size_t)K);
    lay.add(&st.alpha, (size_t)K);
    lay.add(&st.aused, (size_t)K);
    lay.add(&st.sh, pairs);
    lay.add(&st.yh, pairs);
    lay.add(&st.out, (size_t)P + 2);
    lay.add(&st.npairs, n_int);         // [npairs | state | pending | err]: cleared and read back as one range, so one entry
    if (!w->d_block || w->K != K || w->P != P || w->hist != history) {
        if (w->d_block) ROBO_HIP_CHECK(hipFree(w->d_block));
        w->d_block = nullptr;
        ROBO_HIP_CHECK(hipMalloc((void**)&w->d_block, lay.bytes()));
        w->K = K; w->P = P; w->hist = history;
    }
    lay.bind(w->d_block);
    st.state = st.npairs + K;
    st.pending = st.npairs + 2 * K;
    st.err = st.npairs + 3 * K;
    const size_t trace_doubles = (size_t)(n_iters + 1) * K * (2 * (size_t)P + 3);
    if (out_trace) ROBO_TRY(dev_grow(c->stream, &w->d_trace, &w->trace_cap, trace_doubles));
    st.K = K; st.P = P; st.D = D; st.kind = g->kind; st.n = g->n; st.hist = history; st.n_iters = n_iters;
    st.prior_kind = prior_kind;
    st.mean_c = mean_c; st.step0 = step0; st.c1 = c1; st.gtol = gtol;
    if (prior_kind != 0) for (int i = 0; i < (prior_kind == 2 ? 9 : 5); ++i) st.prior_par[i] = prior_par[i];
    st.trace = out_trace ? w->d_trace : nullptr;
    st.d_sp = g->d_bsp; st.d_ism = g->d_bism; st.d_out = g->d_bout; st.d_fail = g->d_bfail; st.d_grad = w->d_out;
    st.d_x2max = g->d_x2max;
    hipStream_t s = c->stream;
    ROBO_HIP_CHECK(hipMemcpyAsync((void*)st.lower, lower, (size_t)P * sizeof(double), hipMemcpyHostToDevice, s));
    ROBO_HIP_CHECK(hipMemcpyAsync((void*)st.upper, upper, (size_t)P * sizeof(double), hipMemcpyHostToDevice, s));
    ROBO_HIP_CHECK(hipMemcpyAsync(st.x, starts, KP * sizeof(double), hipMemcpyHostToDevice, s));
    ROBO_HIP_CHECK(hipMemsetAsync(st.npairs, 0, n_int * sizeof(int), s));
    // (fb.gram_mixed stays set: the trial points are formed on the device, each carries its own FitSample::direct)
    const FitBuffers fb = batch_buffers(g, K, nullptr);     // the likelihood terms are consumed on the device
    const GradBatch gb = grad_buffers(g, K);
    for (int t = 0; t <= n_iters; ++t) {
        ROBO_TRY(launch_hyper_propose(c, st, t, g->d_X, g->d_bXs, g->n, g->n_pad, np * D));
        ROBO_TRY(launch_potrf(g, fb, true));                // gram + factorisation + inverse diagonal blocks
        ROBO_TRY(launch_grad_loglik_batch(g, gb));
        ROBO_TRY(launch_hyper_accept(c, st, t));
    }
    ROBO_TRY(launch_hyper_result(c, st));
    std::vector<double> hres((size_t)P + 2), hx(KP), hf((size_t)K);
    std::vector<int> hint(n_int);
    ROBO_HIP_CHECK(hipMemcpyAsync(hres.data(), st.out, ((size_t)P + 2) * sizeof(double), hipMemcpyDeviceToHost, s));
    ROBO_HIP_CHECK(hipMemcpyAsync(hx.data(), st.x, KP * sizeof(double), hipMemcpyDeviceToHost, s));
    ROBO_HIP_CHECK(hipMemcpyAsync(hf.data(), st.f, (size_t)K * sizeof(double), hipMemcpyDeviceToHost, s));
    ROBO_HIP_CHECK(hipMemcpyAsync(hint.data(), st.npairs, n_int * sizeof(int), hipMemcpyDeviceToHost, s));
    if (out_trace)
        ROBO_HIP_CHECK(hipMemcpyAsync(out_trace, w->d_trace, trace_doubles * sizeof(double), hipMemcpyDeviceToHost, s));
    ROBO_HIP_CHECK(hipStreamSynchronize(s));
    if (hint[3 * (size_t)K] != 0) {
        set_error("factorisation hand-off timed out inside the optimisation (tuning potrf_batch_follow=0 selects the launch-per-phase form)");
        return ROBO_RUNTIME_ERROR;
    }
    memcpy(out_theta, hres.data(), (size_t)P * sizeof(double));
    *out_value = hres[(size_t)P];
    *out_best = (int32_t)hres[(size_t)P + 1];
    if (out_final) memcpy(out_final, hx.data(), KP * sizeof(double));
    if (out_values) memcpy(out_values, hf.data(), (size_t)K * sizeof(double));
    if (out_status) for (int k = 0; k < K; ++k) out_status[k] = hint[(size_t)K + k];
    return ROBO_OK;
}

}  // extern "C"
