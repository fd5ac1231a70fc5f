// C ABI of librobo_hip.so, part 13: Parzen estimators and their log-density ratio (robo_kde_*; the density is stated in
// include/robo_hip.h).  Host-side orchestration only: every number is produced by the kernels in kde.hip and acq.hip.
#include <cmath>
#include <vector>

#include "api_internal.h"
#include "kde_dev.h"

namespace robo {
constexpr const char* KDE_LABEL = "Parzen estimator";

static void kde_free(robo_kde* h) {
    hipFree(h->d_box);
    hipFree(h->mix[0].d_block);
    hipFree(h->mix[1].d_block);
    hipFree(h->d_cand);
    if (h->k) robo_cand_destroy(h->k);
    robo_ctx* c = h->ctx;
    delete h;
    ctx_release(c);
}

static int kde_ready(const robo_kde* h, unsigned need) {
    for (int q = 0; q < 2; ++q)
        if ((need >> q & 1u) && !h->mix[q].set) {
            set_error("Model has to be trained first!");
            return ROBO_NOT_FITTED;
        }
    return ROBO_OK;
}

// the m candidate rows on the device, the results' handle sized for them, the sweep through the mixtures of `need` (bit 0
// good, bit 1 bad) launched in passes of what the workspace holds (asynchronous).  A pass is a multiple of 128 rows, hence
// of the kernel's tile: the passes only move the grid.
static int kde_sweep(robo_kde* h, unsigned need, const double* rows, int64_t m) {
    if (!rows || m < 1) {
        set_error("%s: %lld candidates, must be >= 1, with their rows", KDE_LABEL, (long long)m);
        return ROBO_BAD_ARGUMENT;
    }
    ROBO_TRY(kde_ready(h, need));
    robo_ctx* c = h->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    if (!h->k || h->k->m != m) {
        if (h->k) robo_cand_destroy(h->k);
        h->k = nullptr;
        ROBO_TRY(cand_alloc(c, m, 1, &h->k));
    }
    robo_cand* k = h->k;
    const int D = h->dim;
    ROBO_TRY(dev_grow(c->stream, &h->d_cand, &h->cand_cap, (size_t)m * D));
    ROBO_HIP_CHECK(hipMemcpyAsync(h->d_cand, rows, (size_t)m * D * sizeof(double), hipMemcpyHostToDevice, c->stream));
    KdeMixDev mix[2];
    for (int q = 0; q < 2; ++q) {
        mix[q].psi = h->mix[q].d_psi;
        mix[q].c = h->mix[q].d_c;
        mix[q].npad = (need >> q & 1u) ? h->mix[q].npad : 0;
    }
    int64_t pass = (int64_t)(workspace_bytes(c) / ((size_t)D * sizeof(double))) / NB * NB;
    if (pass < NB) pass = NB;
    const bool ev = phase_events_on(c, k);                // 30 -> 31: the sweep kernel alone
    if (ev) ROBO_TRY(record_phase(c, EV_FOLD_BEGIN));
    for (int64_t p0 = 0; p0 < m; p0 += pass) {
        const int64_t pm = m - p0 < pass ? m - p0 : pass;
        ROBO_TRY(launch_kde_sweep(c, D, h->d_ctr, mix[0], mix[1], h->d_cand + (size_t)p0 * D, pm, k->d_mean + p0, k->d_var + p0,
                                  k->d_acq_sum + p0, need == 3u ? k->d_flags : nullptr));
    }
    return ev ? record_phase(c, EV_FOLD_END) : ROBO_OK;
}
}  // namespace robo

using namespace robo;

extern "C" {

int32_t robo_kde_create(robo_ctx* ctx, int32_t dim, const double* lo, const double* hi, robo_kde** out) {
    if (!ctx || !lo || !hi || !out) return ROBO_BAD_ARGUMENT;
    bool ok = dim >= 1 && dim <= ROBO_KDE_MAX_DIM;
    for (int d = 0; ok && d < dim; ++d) ok = std::isfinite(lo[d]) && std::isfinite(hi[d]) && lo[d] < hi[d];
    if (!ok) {
        set_error("%s: dim %d (1 .. %d) and a box of finite bounds lo < hi are required", KDE_LABEL, dim, ROBO_KDE_MAX_DIM);
        return ROBO_BAD_ARGUMENT;
    }
    ROBO_HIP_CHECK(hipSetDevice(ctx->device));
    robo_kde* h = new robo_kde();
    memset(h, 0, sizeof(*h));
    h->ctx = ctx;
    ctx_retain(ctx);
    h->dim = dim;
    std::vector<double> box(3 * (size_t)dim);
    for (int d = 0; d < dim; ++d) {
        h->lo[d] = box[d] = lo[d];
        h->hi[d] = box[dim + d] = hi[d];
        box[2 * dim + d] = (lo[d] + hi[d]) / 2.0;           // the centre every t = x - centre is taken from
    }
    BlockLayout lay(sizeof(double));
    lay.add(&h->d_lo, (size_t)dim);
    lay.add(&h->d_hi, (size_t)dim);
    lay.add(&h->d_ctr, (size_t)dim);
    int st = dev_alloc(&h->d_box, lay.bytes());
    if (st == ROBO_OK) {
        lay.bind(h->d_box);
        if (hipMemcpy(h->d_box, box.data(), lay.bytes(), hipMemcpyHostToDevice) != hipSuccess) {
            set_error("%s: the box's upload failed", KDE_LABEL);
            st = ROBO_RUNTIME_ERROR;
        }
    }
    if (st != ROBO_OK) {
        kde_free(h);
        return st;
    }
    *out = h;
    return ROBO_OK;
}

int32_t robo_kde_destroy(robo_kde* h) {
    if (!h) return ROBO_OK;
    hipSetDevice(h->ctx->device);
    hipStreamSynchronize(h->ctx->stream);
    kde_free(h);
    return ROBO_OK;
}

int32_t robo_kde_set_mixture(robo_kde* h, int32_t which, const double* mu, const double* hw, int32_t shared_h, const double* w,
                             int64_t n) {
    if (!h || !mu || !hw) return ROBO_BAD_ARGUMENT;
    if ((which != 0 && which != 1) || n < 1 || n > KDE_MAX_N) {
        set_error("%s: mixture %d (0 good, 1 bad) of %lld components (1 .. 2^20)", KDE_LABEL, which, (long long)n);
        return ROBO_BAD_ARGUMENT;
    }
    const int D = h->dim;
    const size_t n_mu = (size_t)n * D, n_h = shared_h ? (size_t)D : n_mu;
    bool ok = true;
    for (size_t e = 0; ok && e < n_mu; ++e) ok = mu[e] >= h->lo[e % D] && mu[e] <= h->hi[e % D];
    for (size_t e = 0; ok && e < n_h; ++e) ok = std::isfinite(hw[e]) && hw[e] > 0.0;
    double sum_w = w ? 0.0 : (double)n;
    for (int64_t j = 0; ok && w && j < n; ++j) {
        ok = std::isfinite(w[j]) && w[j] >= 0.0;
        sum_w += w[j];
    }
    if (!ok || !(sum_w > 0.0) || !std::isfinite(sum_w)) {
        set_error("%s: every mu inside the box, every h > 0 and finite, every weight >= 0 and finite and not all of them 0 "
                  "are required", KDE_LABEL);
        return ROBO_BAD_ARGUMENT;
    }
    robo_ctx* c = h->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    robo_kde::Mix& mx = h->mix[which];
    mx.set = false;
    const int npad = kde_npad(n), K2 = kde_k2(D);
    BlockLayout lay(sizeof(double));
    lay.add(&mx.d_psi, (size_t)npad * K2);
    lay.add(&mx.d_c, (size_t)npad);
    lay.add(&mx.d_mu, n_mu);
    lay.add(&mx.d_h, n_h);
    lay.add(&mx.d_w, w ? (size_t)n : 0);
    ROBO_TRY(dev_grow(c->stream, &mx.d_block, &mx.bytes, lay.bytes()));
    lay.bind(mx.d_block);
    // (pageable sources: the copies have staged them when they return)
    ROBO_HIP_CHECK(hipMemcpyAsync(mx.d_mu, mu, n_mu * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ROBO_HIP_CHECK(hipMemcpyAsync(mx.d_h, hw, n_h * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (w) ROBO_HIP_CHECK(hipMemcpyAsync(mx.d_w, w, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ROBO_TRY(launch_kde_prepare(c, D, h->d_lo, h->d_hi, h->d_ctr, mx.d_mu, mx.d_h, shared_h != 0, w ? mx.d_w : nullptr, sum_w, n,
                                mx.d_psi, mx.d_c));
    ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));
    mx.n = n;
    mx.npad = npad;
    mx.set = true;
    return ROBO_OK;
}

int32_t robo_kde_get_terms(robo_kde* h, int32_t which, double* out_c, double* out_psi) {
    if (!h || !out_c || !out_psi || (which != 0 && which != 1)) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(kde_ready(h, 1u << which));
    robo_ctx* c = h->ctx;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    const robo_kde::Mix& mx = h->mix[which];
    const int D = h->dim, K2 = kde_k2(D);
    std::vector<double> psi((size_t)mx.n * K2);
    ROBO_HIP_CHECK(hipMemcpyAsync(out_c, mx.d_c, (size_t)mx.n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    ROBO_HIP_CHECK(hipMemcpyAsync(psi.data(), mx.d_psi, psi.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (long long j = 0; j < mx.n; ++j) memcpy(out_psi + (size_t)j * 2 * D, psi.data() + (size_t)j * K2, 2 * D * sizeof(double));
    return ROBO_OK;
}

int32_t robo_kde_logpdf(robo_kde* h, int32_t which, const double* rows, int64_t m, double* out_logp) {
    if (!h || !out_logp || (which != 0 && which != 1)) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(kde_sweep(h, 1u << which, rows, m));
    return finish_call(h->k, KDE_LABEL, ROBO_OK, {{out_logp, which ? h->k->d_var : h->k->d_mean, (size_t)m * sizeof(double)}});
}

int32_t robo_kde_ratio_eval_cand(robo_kde* h, const double* rows, int64_t m, double* out_ratio, double* out_logl, double* out_logg,
                                 double* out_max, int64_t* out_argmax, uint32_t* out_flags) {
    if (!h || !out_max || !out_argmax || !out_flags) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(kde_sweep(h, 3u, rows, m));
    robo_cand* k = h->k;
    const size_t bytes = (size_t)m * sizeof(double);
    // the argmax by the existing reduction (np.argmax: first index, NaN maximal); it copies the ratio into k->d_acq unchanged
    ROBO_TRY(clear_flags_on_error(k, launch_argmax(k, k->d_acq_sum, 1.0)));
    ROBO_TRY(finish_call(k, KDE_LABEL, ROBO_OK, {{out_logl, k->d_mean, bytes}, {out_logg, k->d_var, bytes}}, false));
    return clear_flags_on_error(k, acq_read_back(k, k->d_acq, out_ratio, out_max, out_argmax, out_flags));
}

}  // extern "C"
