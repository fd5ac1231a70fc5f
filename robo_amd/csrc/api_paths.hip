// C ABI of librobo_hip.so, part 7: pathwise posterior samples (robo_paths_create, robo_paths_eval_cand, robo_paths_destroy;
// the rule is stated in include/robo_hip.h).  Host-side orchestration only: every number is produced by the kernels in
// paths.hip (and scale_inputs_kernel).
#include <cmath>
#include <vector>

#include "api_internal.h"
#include "paths.h"

namespace robo {
constexpr const char* PATHS_LABEL = "posterior sample paths";

static bool all_finite(const double* a, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(a[i])) return false;
    return true;
}

static void paths_free(robo_paths* p) {
    hipFree(p->d_Xs);
    hipFree(p->d_ism);
    hipFree(p->d_alpha);
    hipFree(p->d_omega);
    hipFree(p->d_phase);
    hipFree(p->d_w);
    hipFree(p->d_part_val);
    hipFree(p->d_part_idx);
    hipFree(p->d_best_val);
    hipFree(p->d_best_idx);
    hipFree(p->d_flags);
    robo_ctx* c = p->ctx;
    delete p;
    ctx_release(c);
}

// what every launch of the path kernel on this object shares
static PathsArgs paths_args(const robo_paths* p) {
    PathsArgs a;
    memset(&a, 0, sizeof(a));
    a.Xs = p->d_Xs;
    a.alpha = p->d_alpha;
    a.n_tiles = p->n_pad / PT;
    a.ld_alpha = p->n_pad;
    a.omega = p->d_omega;
    a.phase = p->d_phase;
    a.w = p->d_w;
    a.f_tiles = p->F_pad / PT;
    a.ld_w = p->F_pad;
    a.S = p->S;
    a.ns = p->S_pad / PATHS_SW;
    a.cp = p->cov;
    a.fscale = p->fscale;
    a.mean_c = p->mean_c;
    a.y_mean = p->y_mean;
    a.y_std = p->y_std;
    a.flags = p->d_flags;
    return a;
}

// allocations, uploads and the launches of robo_paths_create; the caller synchronises and frees the temporaries
static int paths_build(robo_gp* g, robo_paths* p, const double* omega, const double* phase, const double* w, const double* eps,
                       std::vector<double>& h_omega, std::vector<double>& h_w, double** d_eps, double** d_tmp, double** d_r,
                       double** d_ka) {
    robo_ctx* c = g->ctx;
    hipStream_t st = c->stream;
    const int D = p->dim, n = p->n, n_pad = p->n_pad, F = p->F, F_pad = p->F_pad, S = p->S, S_pad = p->S_pad;
    ROBO_TRY(dev_alloc(&p->d_Xs, (size_t)n_pad * D));
    ROBO_TRY(dev_alloc(&p->d_ism, (size_t)D));
    ROBO_TRY(dev_alloc(&p->d_alpha, (size_t)S_pad * n_pad));
    ROBO_TRY(dev_alloc(&p->d_omega, (size_t)F_pad * D));
    ROBO_TRY(dev_alloc(&p->d_phase, (size_t)F_pad));
    ROBO_TRY(dev_alloc(&p->d_w, (size_t)S_pad * F_pad));
    ROBO_TRY(dev_alloc(&p->d_best_val, (size_t)S));
    ROBO_TRY(dev_alloc(&p->d_best_idx, (size_t)S));
    ROBO_TRY(dev_alloc(&p->d_flags, 4));
    ROBO_TRY(dev_alloc(d_eps, (size_t)S * n));
    ROBO_TRY(dev_alloc(d_tmp, (size_t)S_pad * n_pad));
    ROBO_TRY(dev_alloc(d_r, (size_t)S_pad * n_pad));
    ROBO_TRY(dev_alloc(d_ka, (size_t)S_pad * n_pad));
    // pad features: frequency 0, phase 0, weight 0; pad paths: weight 0 everywhere
    h_omega.assign((size_t)F_pad * D + F_pad, 0.0);
    memcpy(h_omega.data(), omega, (size_t)F * D * sizeof(double));
    memcpy(h_omega.data() + (size_t)F_pad * D, phase, (size_t)F * sizeof(double));
    h_w.assign((size_t)S_pad * F_pad, 0.0);
    for (int s = 0; s < S; ++s) memcpy(h_w.data() + (size_t)s * F_pad, w + (size_t)s * F, (size_t)F * sizeof(double));
    ROBO_HIP_CHECK(hipMemcpyAsync(p->d_omega, h_omega.data(), (size_t)F_pad * D * sizeof(double), hipMemcpyHostToDevice, st));
    ROBO_HIP_CHECK(hipMemcpyAsync(p->d_phase, h_omega.data() + (size_t)F_pad * D, (size_t)F_pad * sizeof(double),
                                  hipMemcpyHostToDevice, st));
    ROBO_HIP_CHECK(hipMemcpyAsync(p->d_w, h_w.data(), h_w.size() * sizeof(double), hipMemcpyHostToDevice, st));
    ROBO_HIP_CHECK(hipMemcpyAsync(*d_eps, eps, (size_t)S * n * sizeof(double), hipMemcpyHostToDevice, st));
    ROBO_HIP_CHECK(hipMemcpyAsync(p->d_Xs, g->d_Xs, (size_t)n_pad * D * sizeof(double), hipMemcpyDeviceToDevice, st));
    ROBO_HIP_CHECK(hipMemcpyAsync(p->d_ism, g->d_theta, (size_t)D * sizeof(double), hipMemcpyDeviceToDevice, st));
    ROBO_HIP_CHECK(hipMemsetAsync(p->d_alpha, 0, (size_t)S_pad * n_pad * sizeof(double), st));
    ROBO_HIP_CHECK(hipMemsetAsync(p->d_flags, 0, 4 * sizeof(unsigned), st));
    // Phi_X w at the training rows by the path kernel itself (the feature pass alone, untransformed), into alpha's rows
    PathsArgs a = paths_args(p);
    a.X = p->d_Xs;
    a.c0 = 0;
    a.m = n_pad;
    a.n_tiles = 0;
    a.raw = 1;
    a.out = p->d_alpha;
    a.ld_out = n_pad;
    ROBO_TRY(launch_paths(c, a, n_pad));
    ROBO_TRY(launch_paths_rhs(c, p->d_alpha, g->d_y, *d_eps, S, n, n_pad, g->mean_c, std::sqrt(g->noise)));
    const size_t bytes = (size_t)S_pad * n_pad * sizeof(double);
    ROBO_HIP_CHECK(hipMemcpyAsync(*d_r, p->d_alpha, bytes, hipMemcpyDeviceToDevice, st));
    ROBO_TRY(launch_paths_solve(c, g->d_K, n_pad, g->d_Linv, n, S, p->d_alpha, *d_tmp));
    // one step of iterative refinement against K itself: K alpha at the training rows by the path kernel (the data pass
    // alone, the diagonal exact), rho = r - (K + noise) alpha, alpha += L^-T L^-1 rho
    ROBO_HIP_CHECK(hipMemsetAsync(*d_ka, 0, bytes, st));
    a.n_tiles = n_pad / PT;
    a.f_tiles = 0;
    a.self = 1;
    a.out = *d_ka;
    ROBO_TRY(launch_paths(c, a, n_pad));
    ROBO_TRY(launch_paths_residual(c, *d_ka, *d_r, p->d_alpha, S, n, n_pad, g->noise));
    ROBO_TRY(launch_paths_solve(c, g->d_K, n_pad, g->d_Linv, n, S, *d_ka, *d_tmp));
    return launch_paths_add(c, p->d_alpha, *d_ka, S, n_pad);
}

}  // namespace robo

using namespace robo;

extern "C" {

int32_t robo_paths_create(robo_gp* g, int32_t F, int32_t S, const double* omega, const double* phase, const double* w,
                          const double* eps, robo_paths** out) {
    if (!g || !omega || !phase || !w || !eps || !out) {
        set_error("%s: a NULL pointer among the GP, omega, phase, w, eps and the result", PATHS_LABEL);
        return ROBO_BAD_ARGUMENT;
    }
    *out = nullptr;
    if (g->kind == ROBO_KERNEL_FABOLAS) {
        set_error("%s: the Fabolas kernel is not stationary (no spectral features): matern52 and rbf only", PATHS_LABEL);
        return ROBO_BAD_ARGUMENT;
    }
    if (F < 1 || F > ROBO_PATHS_MAX_FEATURES || S < 1 || S > ROBO_PATHS_MAX) {
        set_error("%s: F = %d features, must be in [1, %d], and S = %d paths, must be in [1, %d]", PATHS_LABEL, F,
                  ROBO_PATHS_MAX_FEATURES, S, ROBO_PATHS_MAX);
        return ROBO_BAD_ARGUMENT;
    }
    if (!g->fitted) {
        set_error("Model has to be trained first!");
        return ROBO_NOT_FITTED;
    }
    if (!all_finite(omega, (size_t)F * g->dim) || !all_finite(phase, (size_t)F) || !all_finite(w, (size_t)S * F) ||
        !all_finite(eps, (size_t)S * g->n)) {
        set_error("%s: a non-finite entry in omega, phase, w or eps", PATHS_LABEL);
        return ROBO_BAD_ARGUMENT;
    }
    robo_ctx* c = g->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    robo_paths* p = new robo_paths();
    memset(p, 0, sizeof(*p));
    p->ctx = c;
    ctx_retain(c);
    p->kind = g->kind;
    p->dim = g->dim;
    p->n = g->n;
    p->n_pad = g->n_pad;
    p->F = F;
    p->F_pad = round_up(F, PT);
    p->S = S;
    p->S_pad = round_up(S, PATHS_SW);
    p->cov = g->cov;
    p->mean_c = g->mean_c;
    p->y_mean = g->y_mean;
    p->y_std = g->y_std;
    p->fscale = std::sqrt(2.0 * g->cov.amp / (double)F);
    std::vector<double> h_omega, h_w;              // staged uploads: alive until the synchronisation below
    double *d_eps = nullptr, *d_tmp = nullptr, *d_r = nullptr, *d_ka = nullptr;
    int st = paths_build(g, p, omega, phase, w, eps, h_omega, h_w, &d_eps, &d_tmp, &d_r, &d_ka);
    const hipError_t e = hipStreamSynchronize(c->stream);          // the one synchronisation of the call
    hipFree(d_eps);
    hipFree(d_tmp);
    hipFree(d_r);
    hipFree(d_ka);
    if (st == ROBO_OK && e != hipSuccess) {
        set_error("%s: %s", PATHS_LABEL, hipGetErrorString(e));
        st = ROBO_RUNTIME_ERROR;
    }
    if (st != ROBO_OK) {
        paths_free(p);
        return st;
    }
    *out = p;
    return ROBO_OK;
}

int32_t robo_paths_eval_cand(robo_paths* p, robo_cand* k, double* out_values, double* out_min, int64_t* out_argmin,
                             uint32_t* out_flags) {
    if (!p || !k || !out_min || !out_argmin || !out_flags) {
        set_error("%s: a NULL pointer among the paths, the candidates, out_min, out_argmin and out_flags", PATHS_LABEL);
        return ROBO_BAD_ARGUMENT;
    }
    if (k->ctx != p->ctx) {
        set_error("%s: the paths and the candidates must live on one context", PATHS_LABEL);
        return ROBO_BAD_ARGUMENT;
    }
    if (k->dim != p->dim) {
        set_error("%s: the paths (dim %d) do not match the candidates (dim %d)", PATHS_LABEL, p->dim, k->dim);
        return ROBO_BAD_SHAPE;
    }
    robo_ctx* c = p->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    const int S = p->S;
    // the values of a pass live in the candidate workspace (S <= 64 < n_pad doubles per candidate); without them no
    // workspace is touched and the passes are the same
    int64_t chunk;
    if (out_values) {
        ROBO_TRY(cand_ensure_workspace(k, p->n_pad, false));
        chunk = k->chunk;
    } else {
        chunk = (int64_t)(workspace_bytes(c) / ((size_t)p->n_pad * sizeof(double))) / NB * NB;
        if (chunk < NB) chunk = NB;
        if (chunk > k->m_pad) chunk = k->m_pad;
    }
    const size_t n_part = (size_t)(k->m_pad / PT);
    if (n_part > p->part_cap) {
        if (p->d_part_val) ROBO_HIP_CHECK(hipFree(p->d_part_val));
        if (p->d_part_idx) ROBO_HIP_CHECK(hipFree(p->d_part_idx));
        p->d_part_val = nullptr;
        p->d_part_idx = nullptr;
        p->part_cap = 0;
        ROBO_TRY(dev_alloc(&p->d_part_val, (size_t)S * n_part));
        ROBO_TRY(dev_alloc(&p->d_part_idx, (size_t)S * n_part));
        p->part_cap = n_part;
    }
    k->solved_gen = 0;                             // the handle's scaled rows are this snapshot's from here on
    int st = launch_scale_inputs(c, k->d_Xc, k->d_Xcs, p->d_ism, k->m, k->m_pad, p->dim);
    PathsArgs a = paths_args(p);
    a.X = k->d_Xcs;
    a.m = k->m;
    a.out = out_values ? k->d_V : nullptr;
    a.ld_out = chunk;
    a.part_val = p->d_part_val;
    a.part_idx = p->d_part_idx;
    a.n_part = (long long)n_part;
    // event slots 30 -> 31 bracket the passes of the path kernel, under the condition of slots 24..27
    const bool ev = c->phase_events || k->m_pad > 16384;
    if (ev && st == ROBO_OK && hipEventRecord(c->events[30], c->stream) != hipSuccess) st = ROBO_RUNTIME_ERROR;
    for (int64_t c0 = 0; st == ROBO_OK && c0 < k->m_pad; c0 += chunk) {
        const int64_t cn = k->m_pad - c0 < chunk ? k->m_pad - c0 : chunk;
        a.c0 = c0;
        st = launch_paths(c, a, cn);
        const int64_t live = k->m - c0 < cn ? k->m - c0 : cn;
        for (int s = 0; st == ROBO_OK && out_values && live > 0 && s < S; ++s)
            if (hipMemcpyAsync(out_values + (size_t)s * k->m + c0, k->d_V + (size_t)s * chunk, (size_t)live * sizeof(double),
                               hipMemcpyDeviceToHost, c->stream) != hipSuccess) {
                set_error("%s: read-back of the values failed", PATHS_LABEL);
                st = ROBO_RUNTIME_ERROR;
            }
    }
    if (ev && st == ROBO_OK && hipEventRecord(c->events[31], c->stream) != hipSuccess) st = ROBO_RUNTIME_ERROR;
    if (st == ROBO_OK) st = launch_paths_best(c, p->d_part_val, p->d_part_idx, (long long)n_part, S, p->d_best_val, p->d_best_idx);
    unsigned flags = 0;
    std::vector<long long> idx((size_t)S);
    if (st == ROBO_OK) {
        hipError_t e = hipMemcpyAsync(out_min, p->d_best_val, (size_t)S * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(idx.data(), p->d_best_idx, (size_t)S * sizeof(long long), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&flags, p->d_flags, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) {
            set_error("%s: read-back failed: %s", PATHS_LABEL, hipGetErrorString(e));
            st = ROBO_RUNTIME_ERROR;
        }
    }
    hipMemsetAsync(p->d_flags, 0, 4 * sizeof(unsigned), c->stream);         // cleared for the next call, failed or not
    const hipError_t e = hipStreamSynchronize(c->stream);                  // the one synchronisation of the call
    if (st == ROBO_OK && e != hipSuccess) {
        set_error("%s: %s", PATHS_LABEL, hipGetErrorString(e));
        st = ROBO_RUNTIME_ERROR;
    }
    if (st != ROBO_OK) return st;
    for (int s = 0; s < S; ++s) out_argmin[s] = (int64_t)idx[(size_t)s];
    *out_flags = flags;
    return ROBO_OK;
}

int32_t robo_paths_destroy(robo_paths* p) {
    if (!p) return ROBO_OK;
    hipSetDevice(p->ctx->device);
    hipStreamSynchronize(p->ctx->stream);
    paths_free(p);
    return ROBO_OK;
}

}  // extern "C"
