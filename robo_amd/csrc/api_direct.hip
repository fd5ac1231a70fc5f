// C ABI of librobo_hip.so: the DIRECT maximiser of a closed-form acquisition (robo_acq_direct, robo_acq_direct_marginal; the
// rule is stated in include/robo_hip.h).  Host-side orchestration only: every number is produced by the kernels in direct.hip
// and the posterior's own.
//
//   dir_init_kernel, per model predict_scaled, dir_divide_kernel(0)
//   ->  T x [ dir_classmin_kernel, dir_select_kernel, per model predict_scaled on its kept handle, dir_divide_kernel ]
//   ->  dir_classmin_kernel, dir_result_kernel
//
// Every launch is enqueued before the first one has run, which is what the fixed batch of B rows is for; nothing between
// the first launch and the read-back touches the host.
#include <cmath>
#include <vector>

#include "api_internal.h"

namespace robo {

// delta[j] = 1 / 3^j (j <= LMAX + 1) and d[s], s = k D + p <= LMAX D: every operation rounded once (the rule's "Tables")
static int dir_tables(int D, std::vector<double>* dsz, std::vector<double>* delta) {
#pragma clang fp contract(off)
    delta->resize((size_t)DIR_LMAX + 2);
    double p3 = 1.0;
    for (int j = 0; j <= DIR_LMAX + 1; ++j) {
        (*delta)[j] = 1.0 / p3;
        p3 *= 3.0;                          // exact: 3^25 < 2^53
    }
    dsz->resize((size_t)DIR_LMAX * D + 1);
    for (int s = 0; s <= DIR_LMAX * D; ++s) {
        const int k = s / D, p = s % D;
        const double qk = (*delta)[k] * (*delta)[k], qk1 = (*delta)[k + 1] * (*delta)[k + 1];
        const double a = (double)(D - p) * qk, b = (double)p * qk1;
        (*dsz)[s] = 0.5 * std::sqrt(a + b);
        if (s > 0 && !((*dsz)[s] < (*dsz)[s - 1])) {
            set_error("direct: the size table is not strictly decreasing at class %d (dim %d)", s, D);
            return ROBO_RUNTIME_ERROR;
        }
    }
    return ROBO_OK;
}

static int dir_core(robo_gp* const* gps, int32_t S, int32_t acq_kind, double par, const double* etas, int32_t max_evals,
                    int32_t max_iters, int32_t batch, double eps, int32_t capacity, double* out_x, double* out_value,
                    int32_t* out_evals, int32_t* out_iters, uint32_t* out_flags, double* out_trace) {
    if (!gps || S < 1 || !etas || !out_x) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(check_acq_kind(acq_kind));
    for (int s = 0; s < S; ++s)
        if (!gps[s]) return ROBO_BAD_ARGUMENT;
    robo_gp* g0 = gps[0];
    robo_ctx* c = g0->ctx;
    const int D = g0->dim, B = batch;
    if (D < 1 || D > DIR_MAX_DIM) {
        set_error("direct: dim %d outside 1 .. %d", D, DIR_MAX_DIM);
        return ROBO_BAD_ARGUMENT;
    }
    if (B < 2 * D || B % 2 != 0 || B > 16384 || max_evals < 1 || max_iters < 0 || (capacity != 0 && capacity < 1) ||
        !(eps >= 0.0) || !std::isfinite(eps)) {
        set_error("direct: batch %d (even, %d .. 16384), max_evals %d (>= 1), max_iters %d (>= 0), capacity %d (0 or >= 1), "
                  "eps %g (>= 0, finite)", B, 2 * D, max_evals, max_iters, capacity, eps);
        return ROBO_BAD_ARGUMENT;
    }
    const int64_t cap64 = capacity != 0 ? (int64_t)capacity : (int64_t)max_evals + B;
    if (cap64 > (int64_t)1 << 24) {
        set_error("direct: capacity %lld above 2^24 rectangles", (long long)cap64);
        return ROBO_BAD_ARGUMENT;
    }
    // the kept handle of the first model stands for "the candidates" in the shared checks: same dim, same context
    std::vector<robo_cand*> hs((size_t)S);
    ROBO_TRY(host_cand_rows(g0, B, &hs[0]));
    ROBO_TRY(ensemble_check("direct", 0, gps, S, hs[0]));
    for (int s = 0; s < S; ++s) {
        if (gps[s]->kind == ROBO_KERNEL_FABOLAS) {
            set_error("direct: sample %d has a Fabolas kernel, whose fidelity column is not a box coordinate", s);
            return ROBO_BAD_ARGUMENT;
        }
        for (int t = 0; t < s; ++t)
            if (gps[t] == gps[s]) {
                set_error("direct: samples %d and %d share a model handle (one posterior per handle)", t, s);
                return ROBO_BAD_ARGUMENT;
            }
    }
    const int64_t m_pad = round_up64(B, NB);
    if ((size_t)m_pad * g0->n_pad * sizeof(double) > workspace_bytes(c)) {
        set_error("direct: %d rows of %d columns exceed the solve workspace (ws_bytes)", (int)m_pad, g0->n_pad);
        return ROBO_BAD_SHAPE;
    }

    DirState st;
    memset(&st, 0, sizeof(st));
    std::vector<double> dsz, delta;
    ROBO_TRY(dir_tables(D, &dsz, &delta));
    const int T = max_iters < max_evals / 2 ? max_iters : max_evals / 2, cap = (int)cap64;
    st.D = D;
    st.S = S;
    st.kind = acq_kind;
    st.B = B;
    st.cap = cap;
    st.T = T;
    st.max_evals = max_evals;
    st.n_cls = DIR_LMAX * D + 1;
    st.m_pad = m_pad;
    st.par = par;
    st.eps = eps;

    // The solve follows the library's rule for a batch of B points (decide_winv): decided, W built and the workspaces sized
    // before the first iteration -- nothing below waits for the device.
    std::vector<char> use_w((size_t)S, 0);
    std::vector<CmaModel> models((size_t)S);
    for (int s = 0; s < S; ++s) {
        robo_gp* g = gps[s];
        ROBO_TRY(host_cand_rows(g, B, &hs[s]));
        ROBO_TRY(cand_ensure_workspace(hs[s], g->n_pad, false));
        bool use = false;
        ROBO_TRY(decide_winv(g, hs[s], &use));
        use_w[s] = use ? 1 : 0;
        models[s] = CmaModel{g->d_theta, hs[s]->d_Xcs, hs[s]->d_mean, hs[s]->d_var, etas[s]};
    }

    if (!g0->dir) {
        g0->dir = new DirWork();
        memset(g0->dir, 0, sizeof(DirWork));
    }
    DirWork* wk = g0->dir;
    // one block: 8-byte entries first, then the model records, the 4-byte words, the bytes
    const size_t G = (size_t)(cap + DIR_CHUNK - 1) / DIR_CHUNK, gt = G * st.n_cls;
    BlockLayout lay(16);
    lay.add(&st.c, (size_t)cap * D);
    lay.add(&st.f, (size_t)cap);
    lay.add(&st.x, (size_t)B * D);
    lay.add(&st.fbest, 2);
    lay.add(&st.out, (size_t)D + 4);
    lay.add(&st.dsz, dsz.size());
    lay.add(&st.delta, delta.size());
    lay.add(&st.part_key, gt);
    lay.add(&st.model, (size_t)S);
    lay.add(&st.part_idx, gt);
    lay.add(&st.cls, (size_t)cap);
    lay.add(&st.po_rect, (size_t)B / 2);
    lay.add(&st.po_off, (size_t)B / 2);
    lay.add(&st.hdr, (size_t)DIR_HDR_WORDS);
    lay.add(&st.flags, 1);
    lay.add(&st.lev, (size_t)cap * D);
    ROBO_TRY(dev_grow(c->stream, &wk->d_block, &wk->bytes, lay.bytes()));
    lay.bind(wk->d_block);
    const size_t trace_len = (size_t)(T + 1) * dir_trace_row(D, B) + (size_t)cap * (2 * D + 1);
    if (out_trace) ROBO_TRY(dev_grow(c->stream, &wk->d_trace, &wk->trace_cap, trace_len));
    st.trace = out_trace ? wk->d_trace : nullptr;

    // (dsz, delta and model are const in DirState, the kernels only read them: the uploads cast that away)
    const hipMemcpyKind h2d = hipMemcpyHostToDevice;
    ROBO_HIP_CHECK(hipMemcpyAsync((void*)st.dsz, dsz.data(), dsz.size() * sizeof(double), h2d, c->stream));
    ROBO_HIP_CHECK(hipMemcpyAsync((void*)st.delta, delta.data(), delta.size() * sizeof(double), h2d, c->stream));
    ROBO_HIP_CHECK(hipMemcpyAsync((void*)st.model, models.data(), (size_t)S * sizeof(CmaModel), h2d, c->stream));

    // the centre, the iterations, the winner: launches only
    auto posterior = [&]() {
        int status = ROBO_OK;
        for (int s = 0; status == ROBO_OK && s < S; ++s) status = predict_scaled(gps[s], hs[s], use_w[s] != 0);
        return status;
    };
    int status = launch_dir_init(c, st);
    if (status == ROBO_OK) status = posterior();
    if (status == ROBO_OK) status = launch_dir_divide(c, st, 0);
    for (int t = 1; status == ROBO_OK && t <= T; ++t) {
        status = launch_dir_classmin(c, st, 0);
        if (status == ROBO_OK) status = launch_dir_select(c, st, t);
        if (status == ROBO_OK) status = posterior();
        if (status == ROBO_OK) status = launch_dir_divide(c, st, t);
    }
    if (status == ROBO_OK) status = launch_dir_classmin(c, st, 1);
    if (status == ROBO_OK) status = launch_dir_result(c, st);
    // read-back: the one synchronisation of the call
    std::vector<double> h((size_t)D + 4);
    ROBO_TRY(finish_call(hs[0], "direct", status, {{h.data(), st.out, h.size() * sizeof(double)},
                                                    {out_trace, wk->d_trace, trace_len * sizeof(double)}}));
    memcpy(out_x, h.data(), (size_t)D * sizeof(double));
    if (out_value) *out_value = h[D];
    long long v;
    memcpy(&v, &h[D + 1], sizeof(v));
    if (out_evals) *out_evals = (int32_t)v;
    memcpy(&v, &h[D + 2], sizeof(v));
    if (out_iters) *out_iters = (int32_t)v;
    memcpy(&v, &h[D + 3], sizeof(v));
    if (out_flags) *out_flags = (uint32_t)v;
    return ROBO_OK;
}

}  // namespace robo

using namespace robo;

extern "C" {

int32_t robo_acq_direct(robo_gp* gp, int32_t acq_kind, double par, double eta, int32_t max_evals, int32_t max_iters,
                        int32_t batch, double eps, int32_t capacity, double* out_x, double* out_value, int32_t* out_evals,
                        int32_t* out_iters, uint32_t* out_flags, double* out_trace) {
    return dir_core(&gp, gp ? 1 : 0, acq_kind, par, &eta, max_evals, max_iters, batch, eps, capacity, out_x, out_value,
                    out_evals, out_iters, out_flags, out_trace);
}

int32_t robo_acq_direct_marginal(robo_gp* const* gps, int32_t S, int32_t acq_kind, double par, const double* etas,
                                 int32_t max_evals, int32_t max_iters, int32_t batch, double eps, int32_t capacity,
                                 double* out_x, double* out_value, int32_t* out_evals, int32_t* out_iters,
                                 uint32_t* out_flags, double* out_trace) {
    return dir_core(gps, S, acq_kind, par, etas, max_evals, max_iters, batch, eps, capacity, out_x, out_value, out_evals,
                    out_iters, out_flags, out_trace);
}

}  // extern "C"
