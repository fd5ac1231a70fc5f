// C ABI of librobo_hip.so, part 1: the last error string, contexts and their tuning knobs (see include/robo_hip.h for the
// contract and the reference call sites each entry point replaces).  Host-side orchestration only.
#include <atomic>
#include <cctype>
#include <cstdarg>
#include <cstdlib>
#include <mutex>

#include "api_internal.h"

namespace robo {

static thread_local char g_err[1024] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- tuning knobs: environment -> context, once (robo_ctx_create); robo_ctx_set_tuning afterwards -------------------
struct TuneKey {
    const char* name;          // robo_ctx_set_tuning key; the environment variable is ROBO_<NAME in upper case>
    long long Tuning::*ll;
    int Tuning::*i;
    long long dflt;
};
static const TuneKey TUNE_KEYS[] = {
    {"ws_bytes", &Tuning::ws_bytes, nullptr, (long long)6 << 30},
    {"trsm_small_max", &Tuning::trsm_small_max, nullptr, 16384},
    {"trsm_small_narrow", nullptr, &Tuning::trsm_small_narrow, -1},
    {"trsm_small_deep", nullptr, &Tuning::trsm_small_deep, -1},
    {"trsm_rows", nullptr, &Tuning::trsm_rows, 1},
    {"trsm_pair", nullptr, &Tuning::trsm_pair, 0},
    {"predict_stepwise", nullptr, &Tuning::predict_stepwise, 0},
    {"winv_max", &Tuning::winv_max, nullptr, 32768},
    {"winv_min_blocks", nullptr, &Tuning::winv_min_blocks, 6},
    {"winv_cond_max", &Tuning::winv_cond_max, nullptr, 100000},
    {"winv_rows", nullptr, &Tuning::winv_rows, -1},
    {"winv_kc_shift", nullptr, &Tuning::winv_kc_shift, -1},
    {"winv_gemv", nullptr, &Tuning::winv_gemv, -1},
    {"potrf_fused", nullptr, &Tuning::potrf_fused, 1},
    {"potrf_fused_panels", nullptr, &Tuning::potrf_fused_panels, -1},
    {"potrf_tm4_min", nullptr, &Tuning::potrf_tm4_min, 96},
    {"potrf_max_wg", nullptr, &Tuning::potrf_max_wg, 0},
    {"potrf_group", nullptr, &Tuning::potrf_group, 0},
    {"potrf_tail_split", nullptr, &Tuning::potrf_tail_split, 1},
    {"potrf_follow", nullptr, &Tuning::potrf_follow, 1},
    {"potrf_follow_from", nullptr, &Tuning::potrf_follow_from, -2},
    {"potrf_pub_early", nullptr, &Tuning::potrf_pub_early, 6},
    {"potrf_follow_rows", nullptr, &Tuning::potrf_follow_rows, -1},
    {"potrf_poll_sleep", nullptr, &Tuning::potrf_poll_sleep, 1},
    {"potrf_batch_roll", nullptr, &Tuning::potrf_batch_roll, 0},
    {"potrf_batch_follow", nullptr, &Tuning::potrf_batch_follow, -1},
    {"potrf_batch_tm4_min", nullptr, &Tuning::potrf_batch_tm4_min, 96},
    {"potrf_thin_last", nullptr, &Tuning::potrf_thin_last, 1},
    {"potrf_split", nullptr, &Tuning::potrf_split, 3},
    {"potrf_gram_split", nullptr, &Tuning::potrf_gram_split, 0},
    {"potrf_split_min", nullptr, &Tuning::potrf_split_min, 12},
    {"potrf_lead", nullptr, &Tuning::potrf_lead, -1},
    {"mcmc_block_step", nullptr, &Tuning::mcmc_block_step, 2},
    {"mcmc_fused_tail", nullptr, &Tuning::mcmc_fused_tail, 1},
    {"acq_screen", nullptr, &Tuning::acq_screen, 1},
    {"acq_screen_min", &Tuning::acq_screen_min, nullptr, -1},
    {"acq_screen_keep_max", nullptr, &Tuning::acq_screen_keep_max, 25},
    {"acq_screen_dot", nullptr, &Tuning::acq_screen_dot, -1},
    {"acq_screen_lean", nullptr, &Tuning::acq_screen_lean, -1},
    {"acq_screen_single", nullptr, &Tuning::acq_screen_single, -1},
    {"acq_screen_int", nullptr, &Tuning::acq_screen_int, -1},
    {"acq_screen_fused_tail", nullptr, &Tuning::acq_screen_fused_tail, 1},
    {"trsm_chain", nullptr, &Tuning::trsm_chain, -1},
    {"trsm_chain_max_wg", nullptr, &Tuning::trsm_chain_max_wg, 4},
    {"trsm_chain_spin_limit", &Tuning::trsm_chain_spin_limit, nullptr, -1},
};

static void tune_set(Tuning* t, const TuneKey& k, long long v) {
    if (k.ll) t->*(k.ll) = v;
    else t->*(k.i) = (int)v;
}

void tuning_from_env(Tuning* t) {
    for (const TuneKey& k : TUNE_KEYS) {
        char env[64] = "ROBO_";
        size_t o = strlen(env);
        for (const char* p = k.name; *p && o + 1 < sizeof(env); ++p) env[o++] = (char)toupper((unsigned char)*p);
        env[o] = 0;
        const char* e = getenv(env);
        tune_set(t, k, (e && *e) ? (long long)atof(e) : k.dflt);
    }
    if (t->ws_bytes < 1) t->ws_bytes = (long long)6 << 30;   // callers round down to whole 128-candidate blocks
}

static std::mutex g_ctx_life;
static std::atomic<int> g_ctx_live{0};

static void ctx_free(robo_ctx* c) {
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    for (int i = 0; i < ROBO_EVENT_SLOTS; ++i) hipEventDestroy(c->events[i]);
    if (c->aux_ready) {
        hipEventDestroy(c->ev_fork);
        for (int i = 0; i < ROBO_AUX_STREAMS; ++i) {
            hipStreamSynchronize(c->aux[i]);
            hipStreamDestroy(c->aux[i]);
            hipEventDestroy(c->ev_join[i]);
        }
    }
    hipFree(c->d_scalars);
    hipFree(c->d_fail);
    hipFree(c->d_prog);
    hipHostFree(c->h_pinned);
    if (c->h_chain) hipHostFree(c->h_chain);
    ep_release(c);
    mc_release(c);
    if (c->own_stream) hipStreamDestroy(c->stream);
    delete c;
    --g_ctx_live;
}

void ctx_retain(robo_ctx* c) {
    std::lock_guard<std::mutex> lock(g_ctx_life);
    ++c->users;
}

void ctx_release(robo_ctx* c) {
    bool last;
    {
        std::lock_guard<std::mutex> lock(g_ctx_life);
        last = --c->users == 0 && c->closing;
    }
    if (last) ctx_free(c);
}

int ctx_aux_streams(robo_ctx* c) {
    if (c->aux_ready) return ROBO_OK;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    ROBO_HIP_CHECK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    for (int i = 0; i < ROBO_AUX_STREAMS; ++i) {
        ROBO_HIP_CHECK(hipStreamCreateWithFlags(&c->aux[i], hipStreamNonBlocking));
        ROBO_HIP_CHECK(hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming));
    }
    c->aux_ready = true;
    return ROBO_OK;
}

}  // namespace robo

using namespace robo;

extern "C" {

const char* robo_last_error_string(void) { return g_err; }
const char* robo_version_string(void) { return "robo_hip 0.1 (gfx950, fp64 MFMA)"; }

int32_t robo_device_count(int32_t* out_n) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *out_n = n;
    return ROBO_OK;
}

int32_t robo_ctx_create(int32_t device, void* hip_stream, robo_ctx** out) {
    if (!out) return ROBO_BAD_ARGUMENT;
    ROBO_HIP_CHECK(hipSetDevice(device));
    robo_ctx* c = new robo_ctx();
    memset(c, 0, sizeof(*c));
    c->device = device;
    if (hip_stream) {
        c->stream = (hipStream_t)hip_stream;
        c->own_stream = false;
    } else {
        ROBO_HIP_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    for (int i = 0; i < ROBO_EVENT_SLOTS; ++i) ROBO_HIP_CHECK(hipEventCreate(&c->events[i]));
    {   // internal phase events of robo_gp_fit (slots 19..23): off unless ROBO_PHASE_EVENTS=1 / set_phase_events
        const char* e = getenv("ROBO_PHASE_EVENTS");
        c->phase_events = e && atoi(e) != 0;
    }
    tuning_from_env(&c->tune);   // the only place the tuning variables are read
    hipDeviceProp_t prop;
    ROBO_HIP_CHECK(hipGetDeviceProperties(&prop, device));
    snprintf(c->name, sizeof(c->name), "%s (%s)", prop.name, prop.gcnArchName);
    c->num_cu = prop.multiProcessorCount;
    ROBO_TRY(dev_alloc(&c->d_scalars, 8));
    ROBO_TRY(dev_alloc(&c->d_fail, 4));
    ROBO_TRY(dev_alloc(&c->d_prog, 2 * PROG_STRIDE));
    ROBO_HIP_CHECK(hipHostMalloc((void**)&c->h_pinned, (MAX_DIM + 64) * sizeof(double), 0));
    ++g_ctx_live;
    *out = c;
    return ROBO_OK;
}

int32_t robo_ctx_destroy(robo_ctx* c) {
    if (!c) return ROBO_OK;
    bool now;
    {
        std::lock_guard<std::mutex> lock(g_ctx_life);
        c->closing = true;
        now = c->users == 0;
    }
    if (now) ctx_free(c);        // otherwise with the last handle that lives on it (ctx_release)
    return ROBO_OK;
}

int32_t robo_ctx_live_count(int32_t* out_n) {
    if (!out_n) return ROBO_BAD_ARGUMENT;
    *out_n = g_ctx_live.load();
    return ROBO_OK;
}

int32_t robo_ctx_synchronize(robo_ctx* c) {
    if (!c) return ROBO_BAD_ARGUMENT;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));
    return ROBO_OK;
}

int32_t robo_ctx_device_name(robo_ctx* c, char* buf, int32_t len) {
    if (!buf || len <= 0) return ROBO_BAD_ARGUMENT;
    snprintf(buf, (size_t)len, "%s", c->name);
    return ROBO_OK;
}

int32_t robo_ctx_event_record(robo_ctx* c, int32_t slot) {
    if (slot < 0 || slot >= ROBO_EVENT_SLOTS) return ROBO_BAD_ARGUMENT;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    ROBO_HIP_CHECK(hipEventRecord(c->events[slot], c->stream));
    return ROBO_OK;
}

int32_t robo_ctx_set_phase_events(robo_ctx* c, int32_t on) {
    if (!c) return ROBO_BAD_ARGUMENT;
    c->phase_events = on != 0;
    return ROBO_OK;
}

int32_t robo_ctx_set_tuning(robo_ctx* c, const char* key, int64_t value) {
    if (!c || !key) return ROBO_BAD_ARGUMENT;
    if (strcmp(key, "env") == 0) {          // re-read every ROBO_<NAME> variable
        tuning_from_env(&c->tune);
        return ROBO_OK;
    }
    for (const TuneKey& k : TUNE_KEYS)
        if (strcmp(key, k.name) == 0) {
            tune_set(&c->tune, k, value == INT64_MIN ? k.dflt : (long long)value);
            if (c->tune.ws_bytes < 1) c->tune.ws_bytes = (long long)6 << 30;
            if (strcmp(key, "trsm_chain") == 0) c->chain_off = false;     // re-arms a context that a time-out took off the chain
            return ROBO_OK;
        }
    set_error("robo_ctx_set_tuning: unknown key '%s'", key);
    return ROBO_BAD_ARGUMENT;
}

int32_t robo_ctx_event_elapsed_ms(robo_ctx* c, int32_t a, int32_t b, float* out_ms) {
    if (a < 0 || a >= ROBO_EVENT_SLOTS || b < 0 || b >= ROBO_EVENT_SLOTS || !out_ms) return ROBO_BAD_ARGUMENT;
    ROBO_HIP_CHECK(hipEventSynchronize(c->events[b]));
    ROBO_HIP_CHECK(hipEventElapsedTime(out_ms, c->events[a], c->events[b]));
    return ROBO_OK;
}

}  // extern "C"
