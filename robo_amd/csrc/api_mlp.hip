// C ABI of librobo_hip.so, part 10: a small tanh network trained on the device (robo_mlp_*; the rule is stated in
// include/robo_hip.h).  Host-side orchestration only: every number is produced by the kernels in mlp.hip.
#include <cmath>
#include <vector>

#include "api_internal.h"
#include "blr_dev.h"

namespace robo {
constexpr const char* MLP_LABEL = "tanh network";

static void mlp_free(robo_mlp* h) {
    hipFree(h->d_state);
    hipFree(h->d_pad);
    hipFree(h->d_ctl);
    hipFree(h->d_rows);
    hipFree(h->d_part);
    hipFree(h->d_out);
    robo_ctx* c = h->ctx;
    delete h;
    ctx_release(c);
}

static int mlp_ready(const robo_mlp* h) {
    if (!h->has_params) {
        set_error("%s: the parameters have to be set first", MLP_LABEL);
        return ROBO_NOT_FITTED;
    }
    return ROBO_OK;
}
}  // namespace robo

using namespace robo;

extern "C" {

int32_t robo_mlp_create(robo_ctx* ctx, int32_t dim, int32_t n_layers, int32_t width, robo_mlp** out) {
    if (!ctx || !out) return ROBO_BAD_ARGUMENT;
    if (dim < 1 || dim > ROBO_MLP_MAX_DIM || n_layers < 1 || n_layers > ROBO_MLP_MAX_LAYERS || width < 1 ||
        width > ROBO_MLP_MAX_WIDTH) {
        set_error("%s: dim %d (1 .. %d), %d hidden layers (1 .. %d), width %d (1 .. %d)", MLP_LABEL, dim, ROBO_MLP_MAX_DIM,
                  n_layers, ROBO_MLP_MAX_LAYERS, width, ROBO_MLP_MAX_WIDTH);
        return ROBO_BAD_ARGUMENT;
    }
    ROBO_HIP_CHECK(hipSetDevice(ctx->device));
    robo_mlp* h = new robo_mlp();
    memset(h, 0, sizeof(*h));
    h->ctx = ctx;
    ctx_retain(ctx);
    MlpNet& s = h->net;
    s.dim = dim;
    s.L = n_layers;
    s.H = width;
    s.DP = round_up(dim, 4);
    s.IP = round_up(dim, 16);
    s.HP = round_up(width, 16);
    s.P = mlp_out_off(s) + width + 1;
    int st = dev_alloc(&h->d_state, (size_t)7 * s.P + 1);
    if (st == ROBO_OK) st = dev_alloc(&h->d_pad, (size_t)mlp_pad_len(s));
    if (st == ROBO_OK) st = dev_alloc(&h->d_ctl, 2);
    if (st != ROBO_OK) {
        mlp_free(h);
        return st;
    }
    s.pad = h->d_pad;
    *out = h;
    return ROBO_OK;
}

int32_t robo_mlp_destroy(robo_mlp* h) {
    if (!h) return ROBO_OK;
    hipSetDevice(h->ctx->device);
    hipStreamSynchronize(h->ctx->stream);
    mlp_free(h);
    return ROBO_OK;
}

int32_t robo_mlp_param_count(robo_mlp* h, int64_t* out_P) {
    if (!h || !out_P) return ROBO_BAD_ARGUMENT;
    *out_P = h->net.P;
    return ROBO_OK;
}

int32_t robo_mlp_set_params(robo_mlp* h, const double* params) {
    if (!h || !params) return ROBO_BAD_ARGUMENT;
    const int P = h->net.P;
    for (int i = 0; i < P; ++i)
        if (!std::isfinite(params[i])) {
            set_error("%s: parameter %d is not finite", MLP_LABEL, i);
            return ROBO_BAD_ARGUMENT;
        }
    robo_ctx* c = h->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    std::vector<double> host((size_t)3 * P, 0.0);                // [params | m = 0 | v = 0]
    memcpy(host.data(), params, (size_t)P * sizeof(double));
    ROBO_HIP_CHECK(hipMemcpyAsync(h->d_state, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ROBO_TRY(launch_mlp_pack(c, h->net, h->d_state, h->d_pad));
    ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));
    h->steps = 0;
    h->has_params = true;
    return ROBO_OK;
}

int32_t robo_mlp_get_params(robo_mlp* h, double* out_params) {
    if (!h || !out_params) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(mlp_ready(h));
    robo_ctx* c = h->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    ROBO_HIP_CHECK(hipMemcpyAsync(out_params, h->d_state, (size_t)h->net.P * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));
    return ROBO_OK;
}

int32_t robo_mlp_train(robo_mlp* h, const double* rows, const double* y, int64_t n, int32_t n_steps, double lr, double l2,
                       double* out_loss, double* out_grad, double* out_trace) {
    if (!h || !rows || !y) return ROBO_BAD_ARGUMENT;
    if (n < 1 || n_steps < 0 || !std::isfinite(lr) || !(lr > 0.0) || !std::isfinite(l2) || l2 < 0.0) {
        set_error("%s: %lld rows (>= 1), %d steps (>= 0), learning rate %g (positive, finite), l2 %g (>= 0, finite)", MLP_LABEL,
                  (long long)n, n_steps, lr, l2);
        return ROBO_BAD_ARGUMENT;
    }
    ROBO_TRY(mlp_ready(h));
    robo_ctx* c = h->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    const MlpNet& s = h->net;
    const size_t P = (size_t)s.P, len = (size_t)n * s.dim, stride = P + 1;
    const long long chunks = (n + BLR_CHUNK - 1) / BLR_CHUNK;
    // the partials of one pass: what the workspace holds, at least one chunk; the passes continue one sum in chunk order
    long long pass = (long long)(workspace_bytes(c) / (stride * sizeof(double)));
    pass = pass < 1 ? 1 : pass > MLP_MAX_PASS ? MLP_MAX_PASS : pass;
    if (pass > chunks) pass = chunks;
    const size_t n_loss = (size_t)n_steps + 1, o_loss = 2 * (size_t)n_steps, o_grad = o_loss + n_loss;
    const size_t o_trace = o_grad + (out_grad ? P : 0), total = o_trace + (out_trace ? n_loss * P : 0);
    ROBO_TRY(dev_grow(c->stream, &h->d_rows, &h->rows_cap, len + (size_t)n));
    ROBO_TRY(dev_grow(c->stream, &h->d_part, &h->part_cap, (size_t)pass * stride));
    ROBO_TRY(dev_grow(c->stream, &h->d_out, &h->out_cap, total));
    std::vector<double> corr(2 * (size_t)n_steps + 1);
    for (int t = 0; t < n_steps; ++t) {
        corr[2 * t] = 1.0 - std::pow(0.9, (double)(h->steps + t + 1));
        corr[2 * t + 1] = 1.0 - std::pow(0.999, (double)(h->steps + t + 1));
    }
    int ctl[2] = {0, 0};
    ROBO_HIP_CHECK(hipMemcpyAsync(h->d_rows, rows, len * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ROBO_HIP_CHECK(hipMemcpyAsync(h->d_rows + len, y, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ROBO_HIP_CHECK(hipMemcpyAsync(h->d_ctl, ctl, sizeof(ctl), hipMemcpyHostToDevice, c->stream));
    if (n_steps > 0)
        ROBO_HIP_CHECK(hipMemcpyAsync(h->d_out, corr.data(), o_loss * sizeof(double), hipMemcpyHostToDevice, c->stream));
    MlpTrain a;
    a.net = s;
    a.params = h->d_state;
    a.mom = h->d_state + P;
    a.keep = h->d_state + 3 * P;
    a.g = h->d_state + 6 * P;
    a.rows = h->d_rows;
    a.y = h->d_rows + len;
    a.n = n;
    a.part = h->d_part;
    a.corr = h->d_out;
    a.lr = lr;
    a.l2 = l2;
    a.n_steps = n_steps;
    a.loss = h->d_out + o_loss;
    a.grad0 = out_grad ? h->d_out + o_grad : nullptr;
    a.trace = out_trace ? h->d_out + o_trace : nullptr;
    a.ctl = h->d_ctl;
    const bool ev = phase_events_on(c, nullptr);     // 30 -> 31: every step's kernels
    if (ev) ROBO_TRY(record_phase(c, EV_FOLD_BEGIN));
    if (chunks == 1 && c->tune.mlp_fused > 0) {
        ROBO_TRY(launch_mlp_train_one(c, a));
    } else {
        for (int t = 0; t <= n_steps; ++t)
            for (long long c0 = 0; c0 < chunks; c0 += pass) {
                const int nc = (int)(chunks - c0 < pass ? chunks - c0 : pass);
                const bool one = ev && t == 0 && c0 == 0;        // 28 -> 29: the call's first gradient launch alone
                if (one) ROBO_TRY(record_phase(c, EV_GRAD_BEGIN));
                ROBO_TRY(launch_mlp_grad(c, a, c0, nc));
                if (one) ROBO_TRY(record_phase(c, EV_GRAD_END));
                ROBO_TRY(launch_mlp_step(c, a, nc, c0 == 0, c0 + nc == chunks, t));
            }
    }
    if (ev) ROBO_TRY(record_phase(c, EV_FOLD_END));
    ROBO_TRY(launch_mlp_pack(c, s, h->d_state, h->d_pad));
    ROBO_HIP_CHECK(hipMemcpyAsync(ctl, h->d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, c->stream));
    if (out_loss)
        ROBO_HIP_CHECK(hipMemcpyAsync(out_loss, a.loss, n_loss * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (out_grad) ROBO_HIP_CHECK(hipMemcpyAsync(out_grad, a.grad0, P * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (out_trace)
        ROBO_HIP_CHECK(hipMemcpyAsync(out_trace, a.trace, n_loss * P * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));
    h->steps += ctl[1];
    if (ctl[0] == 1) {
        set_error("%s: the loss at the start parameters is not finite: the rows or the targets hold a NaN or an infinity",
                  MLP_LABEL);
        return ROBO_BAD_ARGUMENT;
    }
    if (ctl[0] != 0) {
        // the device wrote the entries up to the last finite step; what follows is said to be undefined by a NaN
        const double nan = std::nan("");
        for (size_t t = (size_t)ctl[1] + 1; t < n_loss; ++t) {
            if (out_loss) out_loss[t] = nan;
            for (size_t e = 0; out_trace && e < P; ++e) out_trace[t * P + e] = nan;
        }
        set_error("%s: the loss left the finite numbers after step %d of this call; the parameters are those before that step",
                  MLP_LABEL, ctl[1] + 1);
        return ROBO_NUMERIC_ERROR;
    }
    return ROBO_OK;
}

int32_t robo_mlp_forward(robo_mlp* h, const double* rows, int64_t m, double* out_features, double* out_value) {
    if (!h || !rows) return ROBO_BAD_ARGUMENT;
    if (m < 1) {
        set_error("%s: %lld rows, must be >= 1", MLP_LABEL, (long long)m);
        return ROBO_BAD_ARGUMENT;
    }
    ROBO_TRY(mlp_ready(h));
    robo_ctx* c = h->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    const size_t len = (size_t)m * h->net.dim, nf = (size_t)m * (h->net.H + 1);
    ROBO_TRY(dev_grow(c->stream, &h->d_rows, &h->rows_cap, len));
    ROBO_TRY(dev_grow(c->stream, &h->d_out, &h->out_cap, nf + (size_t)m));
    ROBO_HIP_CHECK(hipMemcpyAsync(h->d_rows, rows, len * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ROBO_TRY(launch_mlp_forward(c, h->net, h->d_rows, m, out_features ? h->d_out : nullptr, out_value ? h->d_out + nf : nullptr));
    if (out_features)
        ROBO_HIP_CHECK(hipMemcpyAsync(out_features, h->d_out, nf * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (out_value)
        ROBO_HIP_CHECK(hipMemcpyAsync(out_value, h->d_out + nf, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));
    return ROBO_OK;
}

}  // extern "C"
