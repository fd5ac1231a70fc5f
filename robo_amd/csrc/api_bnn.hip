// C ABI of librobo_hip.so, part 11: BOHAMIANN, a Bayesian neural network sampled by scale-adapted SGHMC on the device
// (robo_bnn_*; the rule is stated in include/robo_hip.h).  Host-side orchestration only: every number is produced by the
// kernels in bnn.hip and acq.hip.
#include <cmath>
#include <vector>

#include "api_internal.h"
#include "bnn_dev.h"

namespace robo {
constexpr const char* BNN_LABEL = "Bayesian neural network";

static void bnn_free(robo_bnn* h) {
    hipFree(h->d_params);
    hipFree(h->d_state);
    hipFree(h->d_samples);
    hipFree(h->d_status);
    hipFree(h->d_pads);
    hipFree(h->d_rows);
    hipFree(h->d_idx);
    hipFree(h->d_xi);
    hipFree(h->d_trace);
    hipFree(h->d_cand);
    hipFree(h->d_ps);
    if (h->k) robo_cand_destroy(h->k);
    robo_ctx* c = h->ctx;
    delete h;
    ctx_release(c);
}

static bool bnn_finite(const double* v, size_t count) {
    for (size_t i = 0; i < count; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// the m candidate rows on the device, the moments' handle sized for them, the sweep launched (asynchronous)
static int bnn_sweep(robo_bnn* h, const double* rows, int64_t m, bool per_sample) {
    if (!rows || m < 1) {
        set_error("%s: %lld candidates, must be >= 1, with their rows", BNN_LABEL, (long long)m);
        return ROBO_BAD_ARGUMENT;
    }
    if (h->n_samples < 1) {
        set_error("%s: the sample table is empty", BNN_LABEL);
        return ROBO_NOT_FITTED;
    }
    robo_ctx* c = h->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    if (!h->k || h->k->m != m) {                     // (as the regression's sweep: a candidate handle holds the moments)
        if (h->k) robo_cand_destroy(h->k);
        h->k = nullptr;
        ROBO_TRY(cand_alloc(c, m, 1, &h->k));
    }
    const size_t len = (size_t)m * h->net.dim;
    ROBO_TRY(dev_grow(c->stream, &h->d_cand, &h->cand_cap, len));
    if (per_sample) ROBO_TRY(dev_grow(c->stream, &h->d_ps, &h->ps_cap, (size_t)h->n_samples * (size_t)m));
    if (h->pads_stale) {
        ROBO_TRY(dev_grow(c->stream, &h->d_pads, &h->pads_cap, (size_t)h->n_samples * mlp_pad_len(h->net)));
        ROBO_TRY(launch_bnn_pack(c, h->net, h->d_samples, h->n_samples, h->d_pads));
        h->pads_stale = false;
    }
    ROBO_HIP_CHECK(hipMemcpyAsync(h->d_cand, rows, len * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const bool ev = phase_events_on(c, h->k);        // 30 -> 31: the sweep kernel alone
    if (ev) ROBO_TRY(record_phase(c, EV_FOLD_BEGIN));
    ROBO_TRY(launch_bnn_sweep(c, h->net, h->d_pads, h->d_samples, h->n_samples, h->d_cand, m, h->y_mean, h->y_std, h->add_noise,
                              h->k->d_mean, h->k->d_var, per_sample ? h->d_ps : nullptr));
    return ev ? record_phase(c, EV_FOLD_END) : ROBO_OK;
}
}  // namespace robo

using namespace robo;

extern "C" {

int32_t robo_bnn_create(robo_ctx* ctx, int32_t dim, int32_t n_layers, int32_t width, int32_t n_chains, robo_bnn** out) {
    if (!ctx || !out) return ROBO_BAD_ARGUMENT;
    if (dim < 1 || dim > ROBO_MLP_MAX_DIM || n_layers < 1 || n_layers > ROBO_MLP_MAX_LAYERS || width < 1 ||
        width > ROBO_MLP_MAX_WIDTH || n_chains < 1 || n_chains > ROBO_BNN_MAX_CHAINS) {
        set_error("%s: dim %d (1 .. %d), %d hidden layers (1 .. %d), width %d (1 .. %d), %d chains (1 .. %d)", BNN_LABEL, dim,
                  ROBO_MLP_MAX_DIM, n_layers, ROBO_MLP_MAX_LAYERS, width, ROBO_MLP_MAX_WIDTH, n_chains, ROBO_BNN_MAX_CHAINS);
        return ROBO_BAD_ARGUMENT;
    }
    ROBO_HIP_CHECK(hipSetDevice(ctx->device));
    robo_bnn* h = new robo_bnn();
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
    h->C = n_chains;
    h->y_std = 1.0;
    const size_t P1 = (size_t)s.P + 1;
    int st = dev_alloc(&h->d_params, (size_t)n_chains * P1);
    if (st == ROBO_OK) st = dev_alloc(&h->d_state, (size_t)n_chains * BNN_ARRAYS * BNN_OWN);
    if (st == ROBO_OK) st = dev_alloc(&h->d_samples, (size_t)ROBO_BNN_MAX_SAMPLES * P1);
    if (st == ROBO_OK) st = dev_alloc(&h->d_status, (size_t)2 * n_chains);
    if (st != ROBO_OK) {
        bnn_free(h);
        return st;
    }
    *out = h;
    return ROBO_OK;
}

int32_t robo_bnn_destroy(robo_bnn* h) {
    if (!h) return ROBO_OK;
    hipSetDevice(h->ctx->device);
    hipStreamSynchronize(h->ctx->stream);
    bnn_free(h);
    return ROBO_OK;
}

int32_t robo_bnn_param_count(robo_bnn* h, int64_t* out_count) {
    if (!h || !out_count) return ROBO_BAD_ARGUMENT;
    *out_count = h->net.P + 1;
    return ROBO_OK;
}

int32_t robo_bnn_set_state(robo_bnn* h, const double* params) {
    if (!h || !params) return ROBO_BAD_ARGUMENT;
    const size_t len = (size_t)h->C * (h->net.P + 1);
    if (!bnn_finite(params, len)) {
        set_error("%s: a start parameter is not finite", BNN_LABEL);
        return ROBO_BAD_ARGUMENT;
    }
    robo_ctx* c = h->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    h->has_state = false;
    std::vector<int> status((size_t)2 * h->C, 0);
    ROBO_HIP_CHECK(hipMemcpyAsync(h->d_params, params, len * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ROBO_HIP_CHECK(hipMemcpyAsync(h->d_status, status.data(), status.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    ROBO_TRY(launch_bnn_fill(c, h->d_state, h->C));
    ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));        // (the caller's array is free again)
    h->steps = 0;
    h->n_samples = 0;
    h->pads_stale = true;
    h->ms_valid = false;
    h->has_state = true;
    return ROBO_OK;
}

int32_t robo_bnn_run(robo_bnn* h, const double* rows, const double* y, int64_t n, int32_t n_steps, int32_t n_burn_in,
                     int32_t keep_every, int32_t batch, double lr, double mdecay, double prior_mu, double prior_s,
                     double prior_lambda, uint64_t seed, const int32_t* idx, const double* xi, double* out_trace,
                     int32_t* out_status) {
    if (!h || !rows || !y) return ROBO_BAD_ARGUMENT;
    if (n < 1 || n > (1 << 30) || n_steps < 0 || n_burn_in < 0 || keep_every < 1 || batch < 1 || batch > ROBO_BNN_MAX_BATCH ||
        !std::isfinite(lr) || !(lr > 0.0) || !std::isfinite(mdecay) || !(mdecay > 0.0) || !std::isfinite(prior_mu) ||
        !(prior_mu > 0.0) || !std::isfinite(prior_s) || !(prior_s > 0.0) || !std::isfinite(prior_lambda) || prior_lambda < 0.0) {
        set_error("%s: %lld rows (1 .. 2^30), %d steps (>= 0), burn-in %d (>= 0), keep_every %d (>= 1), batch %d (1 .. %d); lr %g, "
                  "mdecay %g, the noise prior's mean %g and variance %g must be positive and finite, lambda %g >= 0 and finite",
                  BNN_LABEL, (long long)n, n_steps, n_burn_in, keep_every, batch, ROBO_BNN_MAX_BATCH, lr, mdecay, prior_mu,
                  prior_s, prior_lambda);
        return ROBO_BAD_ARGUMENT;
    }
    const MlpNet& s = h->net;
    const size_t P1 = (size_t)s.P + 1, len = (size_t)n * s.dim, n_idx = (size_t)n_steps * batch;
    const size_t n_xi = (size_t)n_steps * h->C * P1, n_trace = ((size_t)n_steps + 1) * h->C * 5 * P1;
    if (!bnn_finite(rows, len) || !bnn_finite(y, (size_t)n)) {
        set_error("%s: the rows or the targets hold a NaN or an infinity", BNN_LABEL);
        return ROBO_BAD_ARGUMENT;
    }
    for (size_t i = 0; idx && i < n_idx; ++i)
        if (idx[i] < 0 || idx[i] >= n) {
            set_error("%s: row index %d of step %lld is outside 0 .. %lld", BNN_LABEL, idx[i], (long long)(i / batch),
                      (long long)n - 1);
            return ROBO_BAD_ARGUMENT;
        }
    if (!h->has_state) {
        set_error("%s: the start state has to be set first", BNN_LABEL);
        return ROBO_NOT_FITTED;
    }
    robo_ctx* c = h->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    ROBO_TRY(dev_grow(c->stream, &h->d_rows, &h->rows_cap, len + (size_t)n));
    if (idx) ROBO_TRY(dev_grow(c->stream, &h->d_idx, &h->idx_cap, n_idx));
    if (xi) ROBO_TRY(dev_grow(c->stream, &h->d_xi, &h->xi_cap, n_xi));
    if (out_trace) ROBO_TRY(dev_grow(c->stream, &h->d_trace, &h->trace_cap, n_trace));
    ROBO_HIP_CHECK(hipMemcpyAsync(h->d_rows, rows, len * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ROBO_HIP_CHECK(hipMemcpyAsync(h->d_rows + len, y, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (idx && n_idx) ROBO_HIP_CHECK(hipMemcpyAsync(h->d_idx, idx, n_idx * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (xi && n_xi) ROBO_HIP_CHECK(hipMemcpyAsync(h->d_xi, xi, n_xi * sizeof(double), hipMemcpyHostToDevice, c->stream));
    // rows of the trace that a chain which ends early never writes read as NaN
    if (out_trace) ROBO_HIP_CHECK(hipMemsetAsync(h->d_trace, 0xFF, n_trace * sizeof(double), c->stream));
    BnnRun a;
    memset(&a, 0, sizeof(a));
    a.net = s;
    a.C = h->C;
    a.batch = batch;
    a.n = n;
    a.rows = h->d_rows;
    a.y = h->d_rows + len;
    a.params = h->d_params;
    a.state = h->d_state;
    a.samples = h->d_samples;
    a.status = h->d_status;
    a.idx = idx ? h->d_idx : nullptr;
    a.xi = xi ? h->d_xi : nullptr;
    a.trace = out_trace ? h->d_trace : nullptr;
    a.call_t0 = h->steps;
    a.burn = n_burn_in;
    a.keep = keep_every;
    a.s0 = h->n_samples;
    a.keeps0 = bnn_keeps(h->steps, n_burn_in, keep_every);
    const double eps = lr / std::sqrt((double)n);
    a.bd = (double)batch;
    a.eps2 = eps * eps;
    a.eps4 = a.eps2 * a.eps2;
    a.c2 = (2.0 * a.eps2) * mdecay;
    a.mdecay = mdecay;
    a.lam_n = prior_lambda / (double)n;
    a.inv_sn = 1.0 / (prior_s * (double)n);
    a.ln_mu = std::log(prior_mu);
    a.seed = seed;
    const long long t_end = h->steps + n_steps;
    const bool stands = h->ms_valid && h->ms_eps2 == a.eps2 && h->ms_mdecay == mdecay;
    a.form_at = stands ? -1 : (h->steps > n_burn_in ? h->steps : (long long)n_burn_in);
    // launches of bounded length, nothing between them: the weights go through memory there and nowhere else, and they are
    // the same bits in LDS and in memory, so the split does not show
    const long long bound = c->tune.bnn_launch_steps < 1 ? 1 : c->tune.bnn_launch_steps;
    const bool ev = phase_events_on(c, nullptr);     // 30 -> 31: the chain launches
    if (ev) ROBO_TRY(record_phase(c, EV_FOLD_BEGIN));
    long long t = h->steps;
    do {                                             // (n_steps = 0: one launch that writes the trace's only row)
        a.t0 = t;
        a.steps = (int)(t_end - t < bound ? t_end - t : bound);
        a.final = t + a.steps == t_end;
        ROBO_TRY(launch_bnn_chain(c, a));
        t += a.steps;
    } while (t < t_end);
    if (ev) ROBO_TRY(record_phase(c, EV_FOLD_END));
    std::vector<int> status((size_t)2 * h->C);
    ROBO_HIP_CHECK(hipMemcpyAsync(status.data(), h->d_status, status.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (out_trace)
        ROBO_HIP_CHECK(hipMemcpyAsync(out_trace, h->d_trace, n_trace * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));
    long long good = n_steps;
    int first_bad = -1;
    for (int ch = 0; ch < h->C; ++ch) {
        if (out_status) out_status[ch] = status[2 * ch];
        if (status[2 * ch] != 0 && status[2 * ch + 1] < good) {
            good = status[2 * ch + 1];
            first_bad = ch;
        } else if (status[2 * ch] != 0 && first_bad < 0) {
            first_bad = ch;
        }
    }
    if (n_steps > 0 && (h->steps < n_burn_in || (a.form_at >= 0 && a.form_at < t_end))) {
        h->ms_valid = true;
        h->ms_eps2 = a.eps2;
        h->ms_mdecay = mdecay;
    }
    const long long kept = (bnn_keeps(h->steps + good, n_burn_in, keep_every) - a.keeps0) * h->C + h->n_samples;
    h->n_samples = (int)(kept > ROBO_BNN_MAX_SAMPLES ? ROBO_BNN_MAX_SAMPLES : kept);
    h->pads_stale = true;
    h->steps += good;
    if (first_bad >= 0) {
        h->has_state = false;                        // the chains stop here: robo_bnn_set_state starts them again
        set_error("%s: a parameter of chain %d left the finite numbers in step %lld of this call; the %d samples kept before "
                  "that step stay", BNN_LABEL, first_bad, good + 1, h->n_samples);
        return ROBO_NUMERIC_ERROR;
    }
    return ROBO_OK;
}

int32_t robo_bnn_get_samples(robo_bnn* h, int32_t* out_count, double* out_samples) {
    if (!h || !out_count) return ROBO_BAD_ARGUMENT;
    *out_count = h->n_samples;
    if (!out_samples || h->n_samples == 0) return ROBO_OK;
    robo_ctx* c = h->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    ROBO_HIP_CHECK(hipMemcpyAsync(out_samples, h->d_samples, (size_t)h->n_samples * (h->net.P + 1) * sizeof(double),
                                  hipMemcpyDeviceToHost, c->stream));
    ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));
    return ROBO_OK;
}

int32_t robo_bnn_set_samples(robo_bnn* h, int32_t count, const double* samples) {
    if (!h || !samples) return ROBO_BAD_ARGUMENT;
    if (count < 1 || count > ROBO_BNN_MAX_SAMPLES || !bnn_finite(samples, (size_t)count * (h->net.P + 1))) {
        set_error("%s: %d samples (1 .. %d) of finite parameters", BNN_LABEL, count, ROBO_BNN_MAX_SAMPLES);
        return ROBO_BAD_ARGUMENT;
    }
    robo_ctx* c = h->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    ROBO_HIP_CHECK(hipMemcpyAsync(h->d_samples, samples, (size_t)count * (h->net.P + 1) * sizeof(double), hipMemcpyHostToDevice,
                                  c->stream));
    ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));
    h->n_samples = count;
    h->pads_stale = true;
    return ROBO_OK;
}

int32_t robo_bnn_set_output_transform(robo_bnn* h, double y_mean, double y_std, int32_t add_noise) {
    if (!h) return ROBO_BAD_ARGUMENT;
    if (!std::isfinite(y_mean) || !std::isfinite(y_std) || !(y_std > 0.0)) {
        set_error("%s: the output transform needs a finite mean and a positive, finite scale (%g, %g)", BNN_LABEL, y_mean, y_std);
        return ROBO_BAD_ARGUMENT;
    }
    h->y_mean = y_mean;
    h->y_std = y_std;
    h->add_noise = add_noise != 0;
    return ROBO_OK;
}

int32_t robo_bnn_predict(robo_bnn* h, const double* rows, int64_t m, double* out_mean, double* out_var,
                         double* out_per_sample) {
    if (!h || !out_mean || !out_var) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(bnn_sweep(h, rows, m, out_per_sample != nullptr));
    const size_t bytes = (size_t)m * sizeof(double);
    return finish_call(h->k, BNN_LABEL, ROBO_OK, {{out_mean, h->k->d_mean, bytes}, {out_var, h->k->d_var, bytes},
                                                  {out_per_sample, h->d_ps, (size_t)h->n_samples * bytes}});
}

int32_t robo_bnn_acq_eval_cand(robo_bnn* h, int32_t acq_kind, double par, double eta, const double* rows, int64_t m,
                               double* out_acq, double* out_max, int64_t* out_argmax, uint32_t* out_flags) {
    if (!h) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(check_acq_kind(acq_kind));
    ROBO_TRY(bnn_sweep(h, rows, m, false));
    robo_cand* k = h->k;
    ROBO_TRY(clear_flags_on_error(k, launch_acq(h->ctx, k, acq_kind, par, eta, false, false)));
    return clear_flags_on_error(k, acq_read_back(k, k->d_acq, out_acq, out_max, out_argmax, out_flags));
}

}  // extern "C"
