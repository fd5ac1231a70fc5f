// C ABI of librobo_hip.so, part 7: pathwise posterior samples (robo_paths_create, robo_paths_eval_cand, robo_paths_descend,
// robo_paths_refine_cand, robo_paths_destroy; the rule is stated in include/robo_hip.h).  Host-side orchestration only: every
// number is produced by the kernels in paths.hip and paths_refine.hip (and scale_inputs_kernel).
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
    hipFree(p->d_refine);
    hipFree(p->d_trace);
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

constexpr const char* REFINE_LABEL = "refinement of a path's minimiser";

static int paths_check_cand(const robo_paths* p, const robo_cand* k) {
    if (k->ctx != p->ctx) {
        set_error("%s: the paths and the candidates must live on one context", PATHS_LABEL);
        return ROBO_BAD_ARGUMENT;
    }
    if (k->dim != p->dim) {
        set_error("%s: the paths (dim %d) do not match the candidates (dim %d)", PATHS_LABEL, p->dim, k->dim);
        return ROBO_BAD_SHAPE;
    }
    return ROBO_OK;
}

static int paths_check_steps(int n_steps, double step0) {
    if (n_steps < 0 || !(step0 > 0.0) || !(step0 <= 0.5)) {
        set_error("%s: n_steps %d (>= 0), step0 %g (0 < step0 <= 0.5)", REFINE_LABEL, n_steps, step0);
        return ROBO_BAD_ARGUMENT;
    }
    return ROBO_OK;
}

static int paths_check_dim(const robo_paths* p) {
    if (p->dim > PATHS_REFINE_MAX_DIM) {
        set_error("%s: dim = %d, the descent kernel takes at most %d", REFINE_LABEL, p->dim, PATHS_REFINE_MAX_DIM);
        return ROBO_BAD_SHAPE;
    }
    return ROBO_OK;
}

// The sweep of robo_paths_eval_cand: the scaled rows, then the passes of the path kernel over the candidates in chunks, the
// values of a pass copied out behind it when they are asked for.  Leaves the per-group bests of every path in d_part_val /
// d_part_idx (*n_part groups of 64 rows of the whole batch: a chunk is a multiple of NB = 128 rows, so a group never
// straddles two passes) and the NaN flag in d_flags.  Launches and copies only.
static int paths_sweep(robo_paths* p, robo_cand* k, double* out_values, size_t* n_part_out) {
    robo_ctx* c = p->ctx;
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
    *n_part_out = n_part;
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
    const bool ev = phase_events_on(c, k);
    if (ev && st == ROBO_OK) st = record_phase(c, EV_FOLD_BEGIN);
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
    if (ev && st == ROBO_OK) st = record_phase(c, EV_FOLD_END);
    return st;
}

// the end of a call on a paths object: the flag word cleared for the next call, failed or not, and the one synchronisation
static int paths_finish(robo_paths* p, int st) {
    robo_ctx* c = p->ctx;
    hipMemsetAsync(p->d_flags, 0, 4 * sizeof(unsigned), c->stream);
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (st == ROBO_OK && e != hipSuccess) {
        set_error("%s: %s", PATHS_LABEL, hipGetErrorString(e));
        st = ROBO_RUNTIME_ERROR;
    }
    return st;
}

// the refinement's device state for P descents (one block that only grows, laid out here) and room for the trace
static int paths_refine_ensure(robo_paths* p, int P, size_t trace_len) {
    const size_t pd = (size_t)P * p->dim, p8 = (size_t)round_up(P, 8);
    PathsRefineState& rs = p->rs;
    // doubles first, then the 8-byte integers, then the 4-byte words
    BlockLayout lay(16);
    lay.add(&rs.x0, pd);
    lay.add(&rs.x, pd);
    lay.add(&rs.g, pd);
    lay.add(&rs.f, p8);
    lay.add(&rs.sval, p8);
    lay.add(&rs.res, (size_t)p->S * (p->dim + 2));
    lay.add(&rs.start, p8);
    lay.add(&rs.path_of, p8);
    lay.add(&rs.code, p8);
    ROBO_TRY(dev_grow(p->ctx->stream, &p->d_refine, &p->refine_cap, lay.bytes()));
    lay.bind(p->d_refine);
    if (trace_len) ROBO_TRY(dev_grow(p->ctx->stream, &p->d_trace, &p->trace_cap, trace_len));
    return ROBO_OK;
}

// the one launch of the P descents whose starts are in p->rs; ev: event slots 28 -> 29 bracket it
static int paths_descent(robo_paths* p, int P, int T, double step0, const long long* start, bool trace, bool ev) {
    robo_ctx* c = p->ctx;
    const PathsRefineState& rs = p->rs;
    PathsDescentArgs a;
    memset(&a, 0, sizeof(a));
    a.Xs = p->d_Xs;
    a.alpha = p->d_alpha;
    a.n = p->n;
    a.ld_alpha = p->n_pad;
    a.omega = p->d_omega;
    a.phase = p->d_phase;
    a.w = p->d_w;
    a.F = p->F;
    a.ld_w = p->F_pad;
    a.ism = p->d_ism;
    a.cp = p->cov;
    a.fscale = p->fscale;
    a.mean_c = p->mean_c;
    a.y_mean = p->y_mean;
    a.y_std = p->y_std;
    a.P = P;
    a.T = T;
    a.step0 = step0;
    a.path_of = rs.path_of;
    a.start = start;
    a.x0 = rs.x0;
    a.x = rs.x;
    a.f = rs.f;
    a.g = rs.g;
    a.code = rs.code;
    a.trace = trace ? p->d_trace : nullptr;
    a.flags = p->d_flags;
    if (ev) ROBO_TRY(record_phase(c, EV_GRAD_BEGIN));
    ROBO_TRY(launch_paths_descent(c, a));
    if (ev) ROBO_TRY(record_phase(c, EV_GRAD_END));
    return ROBO_OK;
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
    ROBO_TRY(paths_check_cand(p, k));
    robo_ctx* c = p->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    const int S = p->S;
    size_t n_part = 0;
    int st = paths_sweep(p, k, out_values, &n_part);
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
    ROBO_TRY(paths_finish(p, st));
    for (int s = 0; s < S; ++s) out_argmin[s] = (int64_t)idx[(size_t)s];
    *out_flags = flags;
    return ROBO_OK;
}

int32_t robo_paths_descend(robo_paths* p, int32_t P, const int32_t* path_of, const double* x0, int32_t n_steps, double step0,
                           double* out_x, double* out_value, double* out_grad, int32_t* out_code, uint32_t* out_flags,
                           double* out_trace) {
    if (!p || !path_of || !x0 || !out_x || !out_value || !out_flags) {
        set_error("%s: a NULL pointer among the paths, path_of, x0, out_x, out_value and out_flags", REFINE_LABEL);
        return ROBO_BAD_ARGUMENT;
    }
    if (P < 1 || P > ROBO_PATHS_MAX_DESCENTS) {
        set_error("%s: P = %d descents, must be in [1, %d]", REFINE_LABEL, P, ROBO_PATHS_MAX_DESCENTS);
        return ROBO_BAD_ARGUMENT;
    }
    ROBO_TRY(paths_check_steps(n_steps, step0));
    ROBO_TRY(paths_check_dim(p));
    const int D = p->dim, T = n_steps;
    for (int i = 0; i < P; ++i)
        if (path_of[i] < 0 || path_of[i] >= p->S) {
            set_error("%s: path_of[%d] = %d, must be in [0, %d)", REFINE_LABEL, i, path_of[i], p->S);
            return ROBO_BAD_ARGUMENT;
        }
    for (size_t i = 0; i < (size_t)P * D; ++i)
        if (!(x0[i] >= 0.0 && x0[i] <= 1.0)) {
            set_error("%s: coordinate %zu of start %zu is %g, outside the box [0, 1]", REFINE_LABEL, i % D, i / D, x0[i]);
            return ROBO_BAD_ARGUMENT;
        }
    robo_ctx* c = p->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    const size_t trace_len = (size_t)(T + 1) * P * (2 * D + 3);
    ROBO_TRY(paths_refine_ensure(p, P, out_trace ? trace_len : 0));
    const PathsRefineState& rs = p->rs;
    const size_t pd = (size_t)P * D * sizeof(double);
    ROBO_HIP_CHECK(hipMemcpyAsync(rs.x0, x0, pd, hipMemcpyHostToDevice, c->stream));
    ROBO_HIP_CHECK(hipMemcpyAsync(rs.path_of, path_of, (size_t)P * sizeof(int), hipMemcpyHostToDevice, c->stream));
    int st = paths_descent(p, P, T, step0, nullptr, out_trace != nullptr, true);
    unsigned flags = 0;
    if (st == ROBO_OK) {
        hipError_t e = hipMemcpyAsync(out_x, rs.x, pd, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(out_value, rs.f, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && out_grad) e = hipMemcpyAsync(out_grad, rs.g, pd, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && out_code) e = hipMemcpyAsync(out_code, rs.code, (size_t)P * sizeof(int), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && out_trace)
            e = hipMemcpyAsync(out_trace, p->d_trace, trace_len * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&flags, p->d_flags, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) {
            set_error("%s: read-back failed: %s", REFINE_LABEL, hipGetErrorString(e));
            st = ROBO_RUNTIME_ERROR;
        }
    }
    ROBO_TRY(paths_finish(p, st));
    *out_flags = flags;
    return ROBO_OK;
}

int32_t robo_paths_refine_cand(robo_paths* p, robo_cand* k, int32_t n_starts, int32_t n_steps, double step0, double* out_x,
                               double* out_value, int64_t* out_start_index, uint32_t* out_flags, int64_t* out_starts,
                               double* out_trace) {
    if (!p || !k || !out_x || !out_value || !out_start_index || !out_flags) {
        set_error("%s: a NULL pointer among the paths, the candidates, out_x, out_value, out_start_index and out_flags",
                  REFINE_LABEL);
        return ROBO_BAD_ARGUMENT;
    }
    if (n_starts < 1 || n_starts > ROBO_PATHS_MAX_STARTS) {
        set_error("%s: n_starts = %d, must be in [1, %d]", REFINE_LABEL, n_starts, ROBO_PATHS_MAX_STARTS);
        return ROBO_BAD_ARGUMENT;
    }
    ROBO_TRY(paths_check_steps(n_steps, step0));
    ROBO_TRY(paths_check_cand(p, k));
    ROBO_TRY(paths_check_dim(p));
    robo_ctx* c = p->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    const int S = p->S, D = p->dim, K = n_starts, T = n_steps, P = S * K;
    const size_t trace_len = (size_t)(T + 1) * P * (2 * D + 3);
    ROBO_TRY(paths_refine_ensure(p, P, out_trace ? trace_len : 0));
    const PathsRefineState& rs = p->rs;
    size_t n_part = 0;
    int st = paths_sweep(p, k, nullptr, &n_part);
    if (st == ROBO_OK) st = launch_paths_starts(c, p->d_part_val, p->d_part_idx, (long long)n_part, S, K, k->d_Xc, D, rs);
    if (st == ROBO_OK && (T > 0 || out_trace))
        st = paths_descent(p, P, T, step0, rs.start, out_trace != nullptr, phase_events_on(c, k));
    if (st == ROBO_OK) st = launch_paths_winners(c, S, K, D, rs, T == 0, p->d_flags);
    unsigned flags = 0;
    std::vector<double> res((size_t)S * (D + 2));
    std::vector<long long> hs(out_starts ? (size_t)P : 0);
    if (st == ROBO_OK) {
        hipError_t e = hipMemcpyAsync(res.data(), rs.res, res.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && out_starts)
            e = hipMemcpyAsync(hs.data(), rs.start, hs.size() * sizeof(long long), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && out_trace)
            e = hipMemcpyAsync(out_trace, p->d_trace, trace_len * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&flags, p->d_flags, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) {
            set_error("%s: read-back failed: %s", REFINE_LABEL, hipGetErrorString(e));
            st = ROBO_RUNTIME_ERROR;
        }
    }
    ROBO_TRY(paths_finish(p, st));
    for (int s = 0; s < S; ++s) {
        const double* r = res.data() + (size_t)s * (D + 2);
        memcpy(out_x + (size_t)s * D, r, (size_t)D * sizeof(double));
        out_value[s] = r[D];
        long long v;
        memcpy(&v, &r[D + 1], sizeof(v));
        out_start_index[s] = (int64_t)v;
    }
    for (size_t i = 0; i < hs.size(); ++i) out_starts[i] = (int64_t)hs[i];
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
