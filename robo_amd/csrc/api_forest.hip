// C ABI of librobo_hip.so, part 12: the regression forest (robo_rf_*; the rule is stated in include/robo_hip.h).  Host-side
// orchestration only: every number is produced by the kernels in forest.hip and acq.hip.
#include <cmath>
#include <vector>

#include "api_internal.h"
#include "forest_dev.h"

namespace robo {
constexpr const char* RF_LABEL = "Random forest";

static void rf_free(robo_rf* h) {
    hipFree(h->d_data);
    hipFree(h->d_order);
    hipFree(h->d_nodes);
    hipFree(h->d_scr);
    hipFree(h->d_counts);
    hipFree(h->d_idx);
    hipFree(h->d_cand);
    hipFree(h->d_ps);
    if (h->k) robo_cand_destroy(h->k);
    robo_ctx* c = h->ctx;
    delete h;
    ctx_release(c);
}

static int rf_ready(const robo_rf* h) {
    if (!h->fitted) {
        set_error("Model has to be trained first!");
        return ROBO_NOT_FITTED;
    }
    return ROBO_OK;
}

// the m candidate rows on the device, the moments' handle sized for them, the sweep launched (asynchronous)
static int rf_sweep(robo_rf* h, const double* rows, int64_t m, bool per_tree) {
    if (!rows || m < 1) {
        set_error("%s: %lld candidates, must be >= 1, with their rows", RF_LABEL, (long long)m);
        return ROBO_BAD_ARGUMENT;
    }
    ROBO_TRY(rf_ready(h));
    robo_ctx* c = h->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    if (!h->k || h->k->m != m) {                     // (as the regression's sweep: a candidate handle holds the moments)
        if (h->k) robo_cand_destroy(h->k);
        h->k = nullptr;
        ROBO_TRY(cand_alloc(c, m, 1, &h->k));
    }
    const size_t len = (size_t)m * h->dim;
    ROBO_TRY(dev_grow(c->stream, &h->d_cand, &h->cand_cap, len));
    if (per_tree) ROBO_TRY(dev_grow(c->stream, &h->d_ps, &h->ps_cap, (size_t)h->T * (size_t)m));
    ROBO_HIP_CHECK(hipMemcpyAsync(h->d_cand, rows, len * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const bool ev = phase_events_on(c, h->k);        // 30 -> 31: the sweep kernel alone
    if (ev) ROBO_TRY(record_phase(c, EV_FOLD_BEGIN));
    ROBO_TRY(launch_rf_sweep(c, h->d_nodes, h->d_counts, h->stride, h->T, h->dim, h->total_variance, h->d_cand, m,
                             h->k->d_mean, h->k->d_var, per_tree ? h->d_ps : nullptr));
    return ev ? record_phase(c, EV_FOLD_END) : ROBO_OK;
}
}  // namespace robo

using namespace robo;

extern "C" {

int32_t robo_rf_create(robo_ctx* ctx, int32_t dim, int32_t n_trees, int32_t do_bootstrapping, int32_t max_features,
                       int32_t min_samples_split, int32_t min_samples_leaf, int32_t max_depth, double eps_purity,
                       int32_t total_variance, robo_rf** out) {
    if (!ctx || !out) return ROBO_BAD_ARGUMENT;
    if (dim < 1 || dim > ROBO_RF_MAX_DIM || n_trees < 1 || n_trees > ROBO_RF_MAX_TREES || max_features < 1 ||
        max_features > dim || min_samples_split < 1 || min_samples_leaf < 1 || max_depth < 0 || !std::isfinite(eps_purity) ||
        eps_purity < 0.0) {
        set_error("%s: dim %d (1 .. %d), %d trees (1 .. %d), max_features %d (1 .. dim), min_samples_split %d (>= 1), "
                  "min_samples_leaf %d (>= 1), max_depth %d (>= 0), eps_purity %g (>= 0 and finite)", RF_LABEL, dim,
                  ROBO_RF_MAX_DIM, n_trees, ROBO_RF_MAX_TREES, max_features, min_samples_split, min_samples_leaf, max_depth,
                  eps_purity);
        return ROBO_BAD_ARGUMENT;
    }
    ROBO_HIP_CHECK(hipSetDevice(ctx->device));
    robo_rf* h = new robo_rf();
    memset(h, 0, sizeof(*h));
    h->ctx = ctx;
    ctx_retain(ctx);
    h->dim = dim;
    h->T = n_trees;
    h->bootstrap = do_bootstrapping != 0;
    h->max_features = max_features;
    h->min_split = min_samples_split;
    h->min_leaf = min_samples_leaf;
    h->max_depth = max_depth;
    h->eps_purity = eps_purity;
    h->total_variance = total_variance != 0;
    const int st = dev_alloc(&h->d_counts, (size_t)n_trees);
    if (st != ROBO_OK) {
        rf_free(h);
        return st;
    }
    *out = h;
    return ROBO_OK;
}

int32_t robo_rf_destroy(robo_rf* h) {
    if (!h) return ROBO_OK;
    hipSetDevice(h->ctx->device);
    hipStreamSynchronize(h->ctx->stream);
    rf_free(h);
    return ROBO_OK;
}

int32_t robo_rf_fit(robo_rf* h, const double* rows, const double* y, int64_t n, int32_t n_points, uint64_t seed,
                    const int32_t* idx) {
    if (!h || !rows || !y) return ROBO_BAD_ARGUMENT;
    if (n < 1 || n > ROBO_RF_MAX_N || n_points < 1 || n_points > (1 << 20)) {
        set_error("%s: %lld rows (1 .. %d), %d points per tree (1 .. 2^20)", RF_LABEL, (long long)n, ROBO_RF_MAX_N, n_points);
        return ROBO_BAD_ARGUMENT;
    }
    const int D = h->dim, T = h->T, N = (int)n;
    // feature-major rows behind one scan for non-finite entries; the targets' mean in index order
    std::vector<double> data((size_t)D * N + N);
    bool ok = true;
    double sum = 0.0;
    for (int i = 0; i < N; ++i) {
        for (int d = 0; d < D; ++d) {
            const double x = rows[(size_t)i * D + d];
            ok = ok && std::isfinite(x);
            data[(size_t)d * N + i] = x;
        }
        ok = ok && std::isfinite(y[i]);
        data[(size_t)D * N + i] = y[i];
        sum += y[i];
    }
    const double ybar = sum / (double)N;
    if (!ok || !std::isfinite(ybar)) {
        set_error("%s: the rows or the targets hold a NaN or an infinity", RF_LABEL);
        return ROBO_BAD_ARGUMENT;
    }
    const bool draws = h->bootstrap && idx;
    const size_t n_idx = (size_t)T * n_points;
    for (size_t i = 0; draws && i < n_idx; ++i)
        if (idx[i] < 0 || idx[i] >= N) {
            set_error("%s: draw %d of tree %lld is outside 0 .. %d", RF_LABEL, idx[i], (long long)(i / n_points), N - 1);
            return ROBO_BAD_ARGUMENT;
        }
    robo_ctx* c = h->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    h->fitted = false;
    const int stride = 2 * N - 1;
    const size_t list_len = (size_t)D * N;
    ROBO_TRY(dev_grow(c->stream, &h->d_data, &h->data_cap, data.size()));
    ROBO_TRY(dev_grow(c->stream, &h->d_order, &h->order_cap, list_len * (1 + 2 * (size_t)T)));
    ROBO_TRY(dev_grow(c->stream, &h->d_nodes, &h->nodes_cap, (size_t)T * stride));
    ROBO_TRY(dev_grow(c->stream, &h->d_scr, &h->scr_cap, (size_t)T * stride));
    if (draws) ROBO_TRY(dev_grow(c->stream, &h->d_idx, &h->idx_cap, n_idx));
    // (pageable sources: the copies have staged them when they return)
    ROBO_HIP_CHECK(hipMemcpyAsync(h->d_data, data.data(), data.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (draws) ROBO_HIP_CHECK(hipMemcpyAsync(h->d_idx, idx, n_idx * sizeof(int), hipMemcpyHostToDevice, c->stream));
    RfGrow a;
    memset(&a, 0, sizeof(a));
    a.n = N;
    a.D = D;
    a.T = T;
    a.stride = stride;
    a.n_points = n_points;
    a.bootstrap = h->bootstrap;
    a.max_features = h->max_features;
    a.min_split = h->min_split;
    a.min_leaf = h->min_leaf;
    a.max_depth = h->max_depth;
    a.eps_purity = h->eps_purity;
    a.ybar = ybar;
    a.seed = seed;
    a.xt = h->d_data;
    a.y = h->d_data + list_len;
    a.order = h->d_order;
    a.idx = draws ? h->d_idx : nullptr;
    a.lists = h->d_order + list_len;
    a.nodes = h->d_nodes;
    a.counts = h->d_counts;
    a.scr = h->d_scr;
    const bool ev = phase_events_on(c, nullptr);     // 30 -> 31: the presort and the trees
    if (ev) ROBO_TRY(record_phase(c, EV_FOLD_BEGIN));
    ROBO_TRY(launch_rf_presort(c, a.xt, N, D, h->d_order));
    ROBO_TRY(launch_rf_grow(c, a));
    if (ev) ROBO_TRY(record_phase(c, EV_FOLD_END));
    ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));
    h->stride = stride;
    h->fitted = true;
    return ROBO_OK;
}

int32_t robo_rf_get_trees(robo_rf* h, int32_t* out_counts, int32_t* out_stride, robo_rf_node* out_nodes) {
    if (!h || !out_counts || !out_stride) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(rf_ready(h));
    robo_ctx* c = h->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    *out_stride = h->stride;
    ROBO_HIP_CHECK(hipMemcpyAsync(out_counts, h->d_counts, (size_t)h->T * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (out_nodes)
        ROBO_HIP_CHECK(hipMemcpyAsync(out_nodes, h->d_nodes, (size_t)h->T * h->stride * sizeof(robo_rf_node),
                                      hipMemcpyDeviceToHost, c->stream));
    ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));
    return ROBO_OK;
}

int32_t robo_rf_set_trees(robo_rf* h, const int32_t* counts, int32_t stride, const robo_rf_node* nodes) {
    if (!h || !counts || !nodes) return ROBO_BAD_ARGUMENT;
    if (stride < 1 || stride > 2 * ROBO_RF_MAX_N - 1) {
        set_error("%s: a stride of %d nodes, must be in 1 .. %d", RF_LABEL, stride, 2 * ROBO_RF_MAX_N - 1);
        return ROBO_BAD_ARGUMENT;
    }
    for (int t = 0; t < h->T; ++t) {
        bool ok = counts[t] >= 1 && counts[t] <= stride;
        for (int i = 0; ok && i < counts[t]; ++i) {
            const robo_rf_node& nd = nodes[(size_t)t * stride + i];
            ok = std::isfinite(nd.threshold) && std::isfinite(nd.mean) && std::isfinite(nd.var) && nd.feature >= -1 &&
                 nd.feature < h->dim &&
                 (nd.feature < 0 || (nd.left > i && nd.left < counts[t] && nd.right > i && nd.right < counts[t]));
        }
        if (!ok) {
            set_error("%s: tree %d is no valid node table (1 .. %d nodes, features in -1 .. %d, children behind their parent, "
                      "finite numbers)", RF_LABEL, t, stride, h->dim - 1);
            return ROBO_BAD_ARGUMENT;
        }
    }
    robo_ctx* c = h->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    h->fitted = false;
    ROBO_TRY(dev_grow(c->stream, &h->d_nodes, &h->nodes_cap, (size_t)h->T * stride));
    ROBO_HIP_CHECK(hipMemcpyAsync(h->d_nodes, nodes, (size_t)h->T * stride * sizeof(robo_rf_node), hipMemcpyHostToDevice, c->stream));
    ROBO_HIP_CHECK(hipMemcpyAsync(h->d_counts, counts, (size_t)h->T * sizeof(int), hipMemcpyHostToDevice, c->stream));
    ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));        // (the caller's arrays are free again)
    h->stride = stride;
    h->fitted = true;
    return ROBO_OK;
}

int32_t robo_rf_predict(robo_rf* h, const double* rows, int64_t m, double* out_mean, double* out_var, double* out_per_tree) {
    if (!h || !out_mean || !out_var) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(rf_sweep(h, rows, m, out_per_tree != nullptr));
    const size_t bytes = (size_t)m * sizeof(double);
    return finish_call(h->k, RF_LABEL, ROBO_OK, {{out_mean, h->k->d_mean, bytes}, {out_var, h->k->d_var, bytes},
                                                 {out_per_tree, h->d_ps, (size_t)h->T * bytes}});
}

int32_t robo_rf_acq_eval_cand(robo_rf* h, int32_t acq_kind, double par, double eta, const double* rows, int64_t m,
                              double* out_acq, double* out_max, int64_t* out_argmax, uint32_t* out_flags) {
    if (!h) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(check_acq_kind(acq_kind));
    ROBO_TRY(rf_sweep(h, rows, m, false));
    robo_cand* k = h->k;
    ROBO_TRY(clear_flags_on_error(k, launch_acq(h->ctx, k, acq_kind, par, eta, false, false)));
    return clear_flags_on_error(k, acq_read_back(k, k->d_acq, out_acq, out_max, out_argmax, out_flags));
}

}  // extern "C"
