// Host helpers shared by the files that hold C ABI entry points (api_*.hip, refine.hip, batch.hip, mes.hip, hyperopt.hip,
// comm.hip, multi.hip): each is declared here once and defined in the file named above its group.  An ensemble driver reads as
// "ensemble_check, acq_sweep, its own kernels, finish_call"; a driver over several models' posteriors as "models_check, its
// staging, models_fold"; a moments entry point as "moments_handle, upload_rows, its kernel, moments_finish".  The library's
// own event slots have names (common.h RoboEventSlot) and are recorded with record_phase under phase_events_on.  A driver
// that keeps device state between its launches lays its arrays out in one allocation with BlockLayout (block_layout.h); its
// diagnostics trace and every other buffer that only grows go through dev_grow.
#pragma once
#include <functional>
#include <initializer_list>

#include "block_layout.h"
#include "common.h"

namespace robo {

inline size_t workspace_bytes(const robo_ctx* c) { return (size_t)c->tune.ws_bytes; }

template <class T>
inline int dev_alloc(T** p, size_t count) {
    ROBO_HIP_CHECK(hipMalloc((void**)p, (count ? count : 1) * sizeof(T)));
    return ROBO_OK;
}

// A grow-once buffer (diagnostics traces, per-context scratch, a state block that only grows): room for `count` elements,
// never shrinks.  A regrow waits for the work `st` holds before it frees; a failed allocation leaves (nullptr, 0).
template <class T>
inline int dev_grow(hipStream_t st, T** p, size_t* cap, size_t count) {
    if (count <= *cap) return ROBO_OK;
    ROBO_HIP_CHECK(hipStreamSynchronize(st));
    if (*p) ROBO_HIP_CHECK(hipFree(*p));
    *p = nullptr;
    *cap = 0;
    ROBO_HIP_CHECK(hipMalloc((void**)p, count * sizeof(T)));
    *cap = count;
    return ROBO_OK;
}

// ---- api_fit.hip: the batch workspace -----------------------------------------------------------------------------------------
// theta -> (FitSample, 1/sqrt(metric_d)); ROBO_BAD_ARGUMENT for non-finite entries
int theta_to_sample(const robo_gp* g, const double* theta, double mean_c, FitSample* sp, double* ism);
int batch_ensure(robo_gp* g, int S);       // grow the batch workspace to hold S samples at the current n_pad

// ---- api_predict.hip: candidate handles and the posterior ---------------------------------------------------------------------
int cand_alloc(robo_ctx* ctx, int64_t m, int32_t dim, robo_cand** out);       // an empty handle (points not uploaded)
int cand_ensure_workspace(robo_cand* k, int n_pad, bool single_chunk);        // the (chunk x n_pad) solve workspace
int decide_winv(robo_gp* g, const robo_cand* k, bool* use);                   // the solve goes through W = L^-1 (built here)
// fills k->d_mean / d_var (asynchronous); after_chunk(c0, cn) runs while the chunk's V = L^-1 K*^T is in the workspace;
// need_v: the caller consumes V itself, not only its reductions
// allow_chain: small batches may take the chained one-launch solve (trsm_chain.hip).  Only for callers that END IN A
// SYNCHRONISATION OF THEIR OWN and call chain_timed_out behind it (true: repeat the call once -- it runs the launches now)
int predict_core(robo_gp* g, robo_cand* k, bool single_chunk = false,
                 const std::function<int(int64_t, int64_t)>& after_chunk = nullptr, bool need_v = false,
                 bool allow_chain = false);
// the rest of predict_core for points whose scaled rows are in k->d_Xcs already, the solve decided (decide_winv) and the
// workspace sized: launches only
// events: record the phase events 24..27 whatever the batch size (the survivors of a screened large batch)
int predict_scaled(robo_gp* g, robo_cand* k, bool winv, const std::function<int(int64_t, int64_t)>& after_chunk = nullptr,
                   bool need_v = false, bool events = false, bool allow_chain = false);
bool winv_candidate(const robo_gp* g, const robo_cand* k);     // the batch and the factor qualify for the explicit inverse
int predict_samples(robo_gp* const* gps, int32_t S, robo_cand* k, int cap);   // -> rows of k->d_mu_all / d_var_all
int host_cand(robo_gp* g, const double* Xc, int64_t m, robo_cand** out, bool* kept);   // the handle behind host arrays
int host_cand_rows(robo_gp* g, int64_t m, robo_cand** out);     // ... kept and sized for m points, nothing uploaded (m <= 16384)

// ---- api_acq.hip: closed-form acquisitions and what the ensemble drivers share -------------------------------------------------
int check_acq_kind(int kind);
int clear_flags_on_error(robo_cand* k, int status);        // -> status; a failed call leaves no stale flag bits in k
// D2H of (max, argmax, flags) [+ d_vec] and the one synchronisation of the call
int acq_read_back(robo_cand* k, const double* d_vec, double* out_vec, double* out_max, int64_t* out_argmax,
                  uint32_t* out_flags);
// sum over the samples of the acquisition into k->d_acq_sum (asynchronous)
int acq_accumulate(robo_gp* const* gps, int32_t S, int32_t acq_kind, double par, const double* etas, robo_cand* k,
                   bool allow_chain = false);
// the sweep into k->d_acq and the argmax partials (asynchronous): gps[0]'s acquisition, or (marginal) the mean over S samples
int acq_sweep(robo_gp* const* gps, int32_t S, bool marginal, int32_t acq_kind, double par, const double* etas, robo_cand* k,
              bool allow_chain = false);
// screen.hip: what robo_acq_eval_cand and its sharded / multi-device forms run.  want_values = false (the caller takes
// (max, argmax, flags) only): an eligible call screens the batch and solves the survivors alone, leaving the winner in k's
// argmax slots exactly as acq_sweep does; every other call is acq_sweep.
// allow_chain (see predict_core): also for the survivors and the probe.  ROBO_CHAIN_RETRY: the probe's solve gave up at the
// synchronisation behind it -- the caller repeats the call.
constexpr int ROBO_CHAIN_RETRY = 0x7C01;     // internal: never leaves the library
// h_report != nullptr: the caller's next step is acq_read_back(k, ...) into that pinned block; a screened call whose tail is
// fused writes the report there itself and sets k->best_reported
int acq_sweep_best(robo_gp* g, int32_t acq_kind, double par, double eta, robo_cand* k, bool want_values,
                   bool allow_chain = false, double* h_report = nullptr);
// the samples of an ensemble call against the candidates, then hipSetDevice.  `label` opens the messages.
constexpr unsigned ENSEMBLE_MES_VERDICTS = 1;      // an unfitted sample is ROBO_BAD_ARGUMENT naming the sample; no shape checks
constexpr unsigned ENSEMBLE_ONE_KIND_FP64 = 2;     // every sample has the first one's kernel kind and fp64 covariance entries
int ensemble_check(const char* label, unsigned flags, robo_gp* const* gps, int32_t S, const robo_cand* k);
// The end of a driver.  status != ROBO_OK: wait for the stream, clear k's flags, return status.  Otherwise issue the copies
// (dst == nullptr: not asked for) and synchronise once; sync = false leaves that to an acq_read_back that follows.
struct ReadBack {
    void* dst;
    const void* src;
    size_t bytes;
};
int finish_call(robo_cand* k, const char* label, int status, std::initializer_list<ReadBack> copies, bool sync = true);
// A fused call that folds the posteriors of SEVERAL MODELS at one candidate batch into one value per candidate (EHVI: two
// objectives; constrained EI: the objective and its constraints) is models_check, the caller's own staging, models_fold.
// models_check: every model non-null and on the candidates' context (ROBO_BAD_ARGUMENT, "<label>: <the_models> and the
// candidates must live on one context"), of their dimension (ROBO_BAD_SHAPE; shape_error(i) words the message for the
// first model i that is not), fitted (ROBO_NOT_FITTED) -- in this order over all models -- then hipSetDevice.
int models_check(const char* label, const char* the_models, robo_gp* const* gps, int32_t S, const robo_cand* k,
                 const std::function<void(int)>& shape_error);
// models_fold: the S sweeps into rows 0 .. S - 1 of k's sample tables, fold() -- the caller's kernel, values into
// k->d_acq_sum -- between the event slots slot_begin and slot_begin + 1, the argmax, the trace's copy, then (max, argmax,
// flags) [+ the values] and the one synchronisation of the call.
// models_fold_launch: everything of it before the read-back (launches only: the values stay in k->d_acq, the winner in
// k's argmax slots), for a driver that goes on from the fold on the device.
int models_fold_launch(robo_gp* const* gps, int32_t S, robo_cand* k, int slot_begin, const std::function<int()>& fold);
int models_fold(const char* label, robo_gp* const* gps, int32_t S, robo_cand* k, int slot_begin,
                const std::function<int()>& fold, ReadBack trace, double* out_vec, double* out_max, int64_t* out_argmax,
                uint32_t* out_flags);
// a one-dimensional candidate handle holding (mean, var) of any model; failure reads "<what> failed: <hip error>"
int moments_handle(robo_ctx* ctx, const double* mean, const double* var, int64_t m, const char* what, robo_cand** out);
// further host rows of a moments call onto the device (asynchronous unless sync; count == 0: skipped); failure as above
struct UploadRows {
    double* dst;
    const double* src;
    size_t count;
};
int upload_rows(robo_ctx* ctx, const char* what, std::initializer_list<UploadRows> rows, bool sync = false);
// The end of a moments call on moments_handle's temporary handle, which it destroys either way -> status.  status ==
// ROBO_OK: the argmax over k->d_acq_sum (reduce; false: the kernel left its own partials, launch_acq's single form) and
// acq_read_back with its one synchronisation.  Otherwise: wait for the stream.
int moments_finish(robo_cand* k, int status, bool reduce, double* out_vec, double* out_max, int64_t* out_argmax,
                   uint32_t* out_flags);
// dH / (exp(log-cost mean) + overhead) of every candidate into k->d_acq and the argmax partials (asynchronous)
int ig_per_cost_core(robo_gp* g, robo_cand* k, robo_cand* rep, int32_t npts, double sn2, const double* logP,
                     const double* lmb, const double* W, const double* dlogPdMu, const double* dlogPdSigma,
                     const double* dlogPdMudMu, robo_gp* cost_gp, robo_cand* cost_k, double overhead);

// ---- qei.hip: joint Monte-Carlo batch EI -------------------------------------------------------------------------------------
void qei_free(QeiWork* w);      // the state robo_qei_batch_* keeps with a GP (its BatchWork, the scenarios' block, the diagnostics)

// ---- refine.hip: what the refinement drivers share (robo_acq_refine_*, robo_cei_refine_cand) -----------------------------------------
inline size_t refine_trace_len(int K, int T, int D) { return (size_t)(T + 1) * K * (2 * D + 3); }
int refine_check_steps(int32_t n_starts, int32_t n_steps, double step0);      // out of range: ROBO_BAD_ARGUMENT
// K (D + 1) rows of n_pad columns must fit the solve workspace (ROBO_BAD_SHAPE) -> the state block and pseudo-row workspace
// kept with `holder`, sized, the trace buffer grown and bound when asked for
int refine_prepare(robo_gp* holder, int n_pad, int K, int T, bool want_trace, RefineWork** out);
int launch_refine_solve(robo_gp* g, RefineWork* w, int K, double* d_rhs);
// the winner's kernel, the copies (point, value, start, flags [+ starts, trace]) and the one synchronisation of the call
int refine_read_back(robo_cand* k, RefineWork* w, int status, int T, double* out_x, double* out_value,
                     int64_t* out_start_index, uint32_t* out_flags, int64_t* out_starts, double* out_trace);

// ---- comm.hip: the exchange kernels multi.hip reduces with, too ------------------------------------------------------------------
int launch_comm_pack_sum(hipStream_t st, const double* d_part, long long m, int have, const unsigned* d_flags, int status,
                         double* d_send);
int launch_comm_ordered_sum(hipStream_t st, const double* d_recv, long long stride, int world, long long m, double* d_total,
                            unsigned* d_flags, int* h_status);

}  // namespace robo
