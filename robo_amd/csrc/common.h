// Shared declarations of librobo_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/robo_hip.h"

namespace robo {

// ---- tiling constants ---------------------------------------------------------------
// Everything N x N is stored row-major fp64 with leading dimension n_pad, a multiple of
// NB.  NB is the Cholesky panel width, the TRSM block and the GEMM workgroup tile edge.
constexpr int NB = 128;
constexpr int WG = 256;          // threads per workgroup of every tiled kernel (4 wave64)
constexpr double JITTER = 1.25e-12;  // george's diagonal jitter
constexpr int MAX_DIM = 256;
constexpr int PROG_STRIDE = 512;     // progress words per sample: one per panel (n_pad <= 65 536)

// v_mfma_f64_16x16x4_f64 accumulator: 4 f64 per lane
typedef double v4d __attribute__((vector_size(32)));

__device__ __forceinline__ v4d mfma_f64(double a, double b, v4d c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// v_mfma_i32_16x16x64_i8: 16 int8 per lane of A and of B, 4 int32 per lane of C / D, no rounding anywhere.  Lane l holds
// A[row l & 15][k = 16 (l >> 4) + j] and B[k = 16 (l >> 4) + j][column l & 15] in byte j of its four words (little endian), and
// D[row 4 (l >> 4) + r][column l & 15] in register r -- the bf16 map of the 16x16 shape carried over, pinned with asymmetric
// integer data by robo_selftest_mfma_layout (diag/selftest.hip).  Off the device (the interpreter under tests/hipemu) the
// same sum in plain C++ from the wave's shuffles.
typedef int v4i __attribute__((vector_size(16)));

__device__ __forceinline__ int dot_i8x8(long long x, long long y) {
    int s = 0;
    for (int j = 0; j < 8; ++j) s += (int)(signed char)(x >> (8 * j)) * (int)(signed char)(y >> (8 * j));
    return s;
}

__device__ __forceinline__ v4i mfma_i8(v4i a, v4i b, v4i c) {
#ifdef __AMDGCN__
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
#else
    const int l = threadIdx.x & 63;
    const long long a0 = (long long)(((unsigned long long)(unsigned)a[1] << 32) | (unsigned)a[0]);
    const long long a1 = (long long)(((unsigned long long)(unsigned)a[3] << 32) | (unsigned)a[2]);
    const long long b0 = (long long)(((unsigned long long)(unsigned)b[1] << 32) | (unsigned)b[0]);
    const long long b1 = (long long)(((unsigned long long)(unsigned)b[3] << 32) | (unsigned)b[2]);
    v4i d = c;
    for (int gk = 0; gk < 4; ++gk) {
        const long long y0 = __shfl(b0, (l & 15) + 16 * gk), y1 = __shfl(b1, (l & 15) + 16 * gk);
        for (int r = 0; r < 4; ++r) {
            const int src = 4 * (l >> 4) + r + 16 * gk;
            const long long x0 = __shfl(a0, src), x1 = __shfl(a1, src);
            d[r] += dot_i8x8(x0, y0) + dot_i8x8(x1, y1);
        }
    }
    return d;
#endif
}

// Single correctly rounded fp64 operations that are NEVER contracted into a fused multiply-add, for the places whose
// results must equal NumPy's bit for bit (the stretch-move proposal of the hyper-parameter chain, mcmc_dev.h).
// ROCm's __dmul_rn / __dadd_rn / __dsub_rn are the plain operators (__clang_hip_math.h) and hipcc's default
// -ffp-contract=fast-honor-pragmas fuses them: round 5's  c - z (c - s)  was compiled to  v_fma_f64 q = -z t + c  and
// the chains left the reference's after a few hundred steps on the MI355X.  The pragma removes the `contract` flag
// from the operation itself, so it stays unfused wherever it is inlined (tests/test_isa.py checks the machine code).
__device__ __forceinline__ double rn_add(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ double rn_sub(double a, double b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ double rn_mul(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double rn_div(double a, double b) {
#pragma clang fp contract(off)
    return a / b;
}

// ---- hand-offs between workgroups of ONE launch (the factorisation's panel followers, potrf.hip) ------------------------
// Per-XCD L2s are not coherent with each other and a CU's L1 is never refreshed by another CU's stores: a payload another
// workgroup reads in the same launch is stored WRITE-THROUGH (relaxed agent-scope atomics = global_store ... sc1) and read
// with L1-bypassing loads of the same kind; the producer drains its stores (s_waitcnt vmcnt(0)) before ONE lane stores the
// progress word, the consumer polls that one word relaxed (MI355X guide, "inter-workgroup visibility": the sc1 / sc1 form).
__device__ __forceinline__ void st_agent(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double ld_agent(const double* p) {
    return __hip_atomic_load(const_cast<double*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent_u32(unsigned* p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned ld_agent_u32(const unsigned* p) {
    return __hip_atomic_load(const_cast<unsigned*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void add_agent_u32(unsigned* p, unsigned v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The same in 16-byte pieces (the chained solve's tile v_i, trsm_chain.hip): global_store_dwordx4 ... sc1 and
// global_load_dwordx4 ... sc1 at a 16-byte aligned address.  There is no 16-byte atomic to lower to them, so the device forms
// are written out, and the compiler does not count them in vmcnt.  A store has left the CU behind drain_vmem like any other.
// A load's registers are defined only behind a wait the compiler cannot see either, so the loads and their wait are ONE
// statement (early-clobber results: as separate statements the compiler moved a result register between a load and the
// wait): ld_agent2x4 reads four consecutive pieces, in flight together, and returns when every vector-memory operation of
// the wave has completed.  Off the device (the interpreter under tests/hipemu) all of them are plain C++.
__device__ __forceinline__ void st_agent2(double* p, double2 v) {
#ifdef __AMDGCN__
    typedef double v2d __attribute__((ext_vector_type(2)));
    const v2d x = {v.x, v.y};
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(x) : "memory");
#else
    p[0] = v.x;
    p[1] = v.y;
#endif
}
__device__ __forceinline__ void ld_agent2x4(const double* p, double2& a, double2& b, double2& c, double2& d) {
#ifdef __AMDGCN__
    typedef double v2d __attribute__((ext_vector_type(2)));
    v2d x0, x1, x2, x3;
    asm volatile(
        "global_load_dwordx4 %0, %4, off sc1\n\t"
        "global_load_dwordx4 %1, %4, off offset:16 sc1\n\t"
        "global_load_dwordx4 %2, %4, off offset:32 sc1\n\t"
        "global_load_dwordx4 %3, %4, off offset:48 sc1\n\t"
        "s_waitcnt vmcnt(0)"
        : "=&v"(x0), "=&v"(x1), "=&v"(x2), "=&v"(x3)
        : "v"(p)
        : "memory");
    a = make_double2(x0.x, x0.y);
    b = make_double2(x1.x, x1.y);
    c = make_double2(x2.x, x2.y);
    d = make_double2(x3.x, x3.y);
#else
    a = make_double2(p[0], p[1]);
    b = make_double2(p[2], p[3]);
    c = make_double2(p[4], p[5]);
    d = make_double2(p[6], p[7]);
#endif
}
// every vector-memory operation of this wave has completed (vmcnt(0); expcnt / lgkmcnt fields left at their maxima)
__device__ __forceinline__ void drain_vmem() { __builtin_amdgcn_s_waitcnt(0x0F70); }
constexpr long long FOLLOW_SENTINEL = 0x7FF8DEAD00C0FFEELL;   // a NaN no arithmetic produces: "W_77 of this panel is not published yet"
constexpr unsigned PROG_SPIN_LIMIT = 1u << 24;   // bounded spin (~seconds): a hand-off that never arrives ends in a flagged failure

// covariance function of the current theta (see kern_math.h)
struct CovParams {
    int kind;   // robo_kernel_kind
    int dim;    // input dimensions (FABOLAS: the last one is the basis-transformed fidelity u)
    double amp, blr_a, blr_b;
};

// per-theta inputs of one fit; the fit kernels take an array of these and index it with the
// batch coordinate of the grid, so S hyper-parameter samples are factorised by ONE sequence of
// launches (S x more workgroups per launch: the MCMC inner loop of the reference evaluates
// n_hypers/2 independent likelihoods per ensemble half-step)
struct FitSample {
    CovParams cov;
    double noise;    // exp(theta[P-1]) + JITTER, added to the diagonal
    double mean_c;   // constant prior mean
    int direct;      // fp64 stationary kernels: K from direct differences instead of the dot form (gram_needs_direct)
};

// Which of the two fp64 tiles of a stationary kernel builds K (gram_tile.h): the dot form  r2 = |xi|^2 + |xj|^2 - 2 xi.xj
// carries an absolute error of about (D + 3) eps (|xi|^2 + |xj|^2) in r2, which is harmless while the SCALED coordinates
// are O(1) and is not at short length scales or for data far from the origin.  The bound below uses the data extents
// x2max[d] = max_i x_id^2 of the raw inputs (robo_gp_set_data) and the inverse square-root metrics of the theta:
//     (D + 3) eps 2 sum_d ism_d^2 x2max_d  >  GRAM_DIRECT_BOUND   ->   direct differences.
// ONE function for the host (theta_to_sample) and the device (the chain and optimiser kernels form theta themselves), every
// operation rounded once and never contracted, so that every path takes the same tile for the same theta.
constexpr double GRAM_DIRECT_BOUND = 1e-12;
__host__ __device__ inline int gram_needs_direct(int kind, const double* ism, const double* x2max, int D) {
#pragma clang fp contract(off)
    if (kind == ROBO_KERNEL_FABOLAS) return 0;      // the product kernel has no dot form
    double s = 0.0;
    for (int d = 0; d < D; ++d) {
        const double m2 = ism[d] * ism[d];
        const double t = m2 * x2max[d];
        s = s + t;
    }
    const double c = (double)(D + 3) * 4.44089209850062616e-16;     // (D + 3) * 2 * 2^-52
    const double b = c * s;
    return b > GRAM_DIRECT_BOUND ? 1 : 0;           // (a NaN extent -- non-finite data -- stays on the dot form)
}

// one theta as kernel arguments (single-sample fits, gram.hip)
struct ThetaArgs {
    FitSample sp;
    double ism[MAX_DIM];   // 1 / sqrt(metric_d)
};

void set_error(const char* fmt, ...);

#define ROBO_HIP_CHECK(expr)                                                                       \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            robo::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return ROBO_RUNTIME_ERROR;                                                             \
        }                                                                                          \
    } while (0)

#define ROBO_LAUNCH_CHECK()                                                                        \
    do {                                                                                           \
        hipError_t _e = hipGetLastError();                                                         \
        if (_e != hipSuccess) {                                                                    \
            robo::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__, __LINE__); \
            return ROBO_RUNTIME_ERROR;                                                             \
        }                                                                                          \
    } while (0)

#define ROBO_TRY(expr)                \
    do {                              \
        int _s = (expr);              \
        if (_s != ROBO_OK) return _s; \
    } while (0)

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
static inline int64_t round_up64(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

}  // namespace robo

// ---- handle layouts --------------------------------------------------------------------
namespace robo {
// Tuning knobs of a context: read ONCE from the environment when the context is created (ROBO_<NAME>), changed
// afterwards only through robo_ctx_set_tuning -- nothing on the hot path calls getenv.  -1 = automatic.
struct Tuning {
    long long ws_bytes;          // solve workspace per candidate handle (default 6 GiB)
    long long trsm_small_max;    // batches <= this use the 16/32-candidate block-row step
    int trsm_small_narrow;       // -1 auto, 0 / 1 force 32 / 16 candidates per workgroup
    int trsm_small_deep;         // -1 auto, 0 / 1 force 1 / 2 k-tiles per staging stage
    int trsm_rows;               // block rows per launch of the 128-candidate step
    int trsm_pair;               // 1: two block rows per launch on one read of V (trsm_pair_gen_kernel; measured slower: default 0)
    int predict_stepwise;        // 1: cross-gram in memory + trsm_step_kernel (A/B)
    long long winv_max;          // batches <= this (and >= winv_min_blocks block rows) go through W = L^-1 (0: never)
    int winv_min_blocks;
    int winv_gemv;               // explicit-inverse posterior of <= 8 candidates as a matrix-vector product: -1 auto, 0 never
    int winv_kc_shift;           // chunked explicit-inverse product: -1 auto (by batch size), 0 / 1 / 2 = the batch chunk depth, half, quarter
    int winv_rows;               // explicit-inverse product per (tile, block row) over the whole contraction range: -1 auto
                                 // (batches that fill the chip that way), 0 never (chunked units + reduction), 1 always
    long long winv_cond_max;     // ... while cond_inf(L) = |L|_inf |W|_inf stays below this (default 1e5)
    int potrf_fused;             // 0: never fuse the next diagonal block into the trailing update
    int potrf_fused_panels;      // ... also for batches of factors with at most this many panels (0: single fits only; -1 =
                                 // default: while the first step's launch is at most three rounds of CUs -- 26 walkers: N <= 766)
    int potrf_tm4_min, potrf_max_wg, potrf_group;
    int potrf_batch_tm4_min;     // batched updates: 128-row tiles from this many (tiles x samples) on, 32-row tiles below (96;
                                 // tests lower it so that the interpreter reaches the 128-row form at small N)
    int potrf_thin_last;         // batched fit: 32-row tiles for the block row that holds only the augmented row (1; 0 = A/B)
    int potrf_split;             // batched fit: sub-batches on their own streams with staggered group boundaries (1: one stream)
    int potrf_gram_split;        // ... with every sub-batch's gram kernel on its own stream (1) or one launch for all (0)
    int potrf_split_min;         // ... from this many panels on (default 12: N >= 1408)
    int potrf_lead;              // ... first-group size step between sub-batches (-1: G / splits)
    int potrf_tail_split;        // fused step: the ragged last round of 128-row tiles as half / quarter tiles on more workgroups
    int potrf_follow;            // single-theta fit: the panel solve of column k+1 FOLLOWS the diagonal block inside the step
                                 // kernel (progress words, potrf_step_follow_kernel) instead of its own launch (default 1; 0: the launch-per-phase form)
    int potrf_follow_from;       // ... from this step on (-1: the first panel too; -2 = default: by size, launch_potrf)
    int potrf_pub_early;         // ... the diagonal block's helper waves count a published column at once from this interval on
    int potrf_follow_rows;       // ... rows per follower workgroup: 64 (two per block row), 128 (one), -1: by step (launch_potrf)
    int potrf_poll_sleep;        // ... pauses (x 128 cycles) between two polls of a follower
    int potrf_batch_roll;        // ... with the diagonal workgroup's 80-KB rolling layout (two workgroups per CU); 0: the 150-KB image
    int potrf_batch_follow;      // batched fits: diagonal block + panel of a step in one launch, the panel following (-1 = default: up to 17 panels; 0 / 1)
    int mcmc_fused_tail;         // device chain, multi-block factors: likelihood terms + accept test in one launch (1)
    int mcmc_block_step;         // ensemble half-step in ONE launch: 2 (default) every one-block problem, 1 only N <= 63, 0 never
                                 // (a larger value means 2: the two-block form that 3 selected was measured slower and removed)
    int acq_screen;              // argmax-only acquisition calls skip the candidates that cannot win (screen.hip): 1 (default), 0 never
    long long acq_screen_min;    // ... for batches above this many candidates (-1 = default: winv_max, above which the unscreened
                                 // call is the block-row substitution; tests lower it so that the interpreter reaches the screen)
    int acq_screen_keep_max;     // ... while at most this percentage of the batch survives (25); beyond it the plain sweep runs
    int acq_screen_dot;          // ... with the bounds pass's squared distances from the matrix pipe (screen_bounds_dot_kernel): -1
                                 // (default) where the fitted theta's worst-case r2 error stays within SCREEN_DOT_BOUND, 0 never,
                                 // 1 wherever the kind and D permit, whatever the bound (tests)
    int acq_screen_lean;         // ... and that kernel's pairs finished to SD_LEAN_EPS amp instead of to the last bit: -1 (default)
                                 // where the term this adds to delta stays within SCREEN_LEAN_MAX of the prior standard
                                 // deviation, 0 never, 1 wherever the dot kernel runs (tests)
    int acq_screen_single;       // ... and, in front of that pass, the same kernel with a single-precision finish (SD_SINGLE_EPS amp) whose
                                 // survivors are solved when they fit one tile: -1 (default) where the lean finish is selected and the
                                 // term this adds to delta stays within SCREEN_SINGLE_MAX of the prior standard deviation, 0 never, 1
                                 // wherever the lean finish runs, 2 as 1 and robo_acq_screen_bounds returns that stage's bounds (tests)
    int acq_screen_int;          // ... that first stage's squared distances from exact int8 matrix products on a 24-bit grid
                                 // (screen_bounds_dot_int_kernel): -1 (default) where the first stage runs, 8 < D <= 16, the training
                                 // rows have an extent and the stage's whole term, the grid's included, stays within
                                 // SCREEN_SINGLE_MAX; 0 never; 1 wherever the first stage runs and D <= 16
    int acq_screen_fused_tail;   // ... survivors that fit one partial block: output transform, acquisition, argmax, index map and
                                 // report in ONE single-workgroup launch (1, default); 0: the five launches (tests, A/B)
    int trsm_chain;              // small batches on >= 2 block rows: all block rows in ONE launch chained by hand-offs (trsm_chain.hip)
                                 // from the entry points that look at its time-out word: -1 auto (>= 3 block rows, within
                                 // trsm_chain_max_wg), 0 never, 1 wherever legal
    int trsm_chain_max_wg;       // ... auto: while (16-candidate tiles x block rows) <= this many times the CU count (4: measured)
    long long trsm_chain_spin_limit;   // TEST ONLY: polls before a consumer gives up (-1 = PROG_SPIN_LIMIT); 0 also keeps the
                                 // producers from publishing, so that the first wait of a launch fails at its first poll
};
void tuning_from_env(Tuning* t);
}  // namespace robo
struct robo_ctx;
namespace robo {
struct EpWork;                          // ep.hip: grow-once buffers of robo_ep_joint_min
void ep_release(robo_ctx* ctx);         // ... freed with the context
struct McWork;                          // igmc.hip: grow-once buffers and uploaded draws of the Monte-Carlo p_min
void mc_release(robo_ctx* ctx);         // ... freed with the context
int ctx_aux_streams(robo_ctx* ctx);   // api_ctx.hip: create ctx->aux / ev_fork / ev_join once
void ctx_retain(robo_ctx* ctx);        // a handle was created on ctx
void ctx_release(robo_ctx* ctx);       // ... destroyed: frees a closing context with its last handle
}

struct robo_cand;
namespace robo {
// ---- multi-start gradient refinement of an acquisition maximum (refine.hip) ------------------------------------------------
// Radix selection of the K best sweep values: the 96-bit key (order-preserving bits of the value, inverted index) of the
// K-th best candidate is found digit by digit, 8 bits per pass.
struct RefineSel {
    unsigned long long hi;      // value part of the threshold key (the digits fixed so far)
    unsigned lo;                // inverted-index part
    unsigned remaining;         // rank of the threshold among the keys that share the fixed digits
    unsigned keff;              // min(K, candidates whose value is not NaN)
    unsigned count;             // slots handed out by the collect kernel
};
// everything a start carries between two launches; all arrays [K] or [K][D], device memory of one block
struct RefineState {
    int K, D;
    double *x, *f, *g, *alpha;      // accepted point, its value and gradient, current step length
    double *aused;                  // step length the pending trial was made with
    double *y, *ys;                 // pending trial points, raw and scaled by the current sample's metrics
    double *fy, *gy;                // value / gradient of the trial, accumulated over the hyper-parameter samples
    int *frozen, *bad;              // start takes no more steps; some sample saw the variance floor at the trial
    long long* start;               // index in the candidate batch the start came from (-1: slot unused)
    double* sel_val;                // [2][K] selected values: as collected, then sorted
    long long* sel_idx;             // [2][K]
    unsigned* hist;                 // [256] digit counts of the current selection pass
    unsigned* flags;                // ROBO_FLAG_* raised by the refinement
    RefineSel* sel;
    double* out;                    // [D + 4]: point, value, start index, flags, starts in use
    double* trace;                  // (T + 1) x K x (2 D + 3), or nullptr
};
struct RefineWork {
    int K, D;
    ::robo_cand* ws;                // the K (D + 1) pseudo-rows of the solve
    char* d_block;                  // one allocation behind `st`, laid out by refine_alloc's BlockLayout (block_layout.h)
    double* d_trace;
    size_t trace_cap;               // doubles
    RefineState st;
};
int refine_alloc(robo_ctx* ctx, int K, int D, RefineWork** out);
void refine_free(RefineWork* w);               // the state block and the trace; `ws` belongs to the caller

// ---- greedy batch proposals with fantasised picks (batch.hip) -----------------------------------------------------------------
// the state of one selection; all arrays device memory of one block, per-sample arrays [S][m_pad] / [S][n_pad]
constexpr int BATCH_MAX_Q = 1024;   // picks per call: the c_t history is S x q x m doubles
struct BatchState {
    int S, q, qcap;                 // qcap: picks the history arrays were sized for
    long long m, m_pad;
    double *mu_lat, *var_lat;       // latent moments of every candidate (before the output transform, never floored)
    double* mean_t;                 // transformed mean: the sweep's own bits until a conditioning step moves the mean
    double *w, *v, *beta;           // k_*(x_j) -> L^-1 k_*(x_j) -> K^-1 k_*(x_j)
    double* chist;                  // [S][qcap][m_pad] c_t(x) of every conditioning step so far
    double* dhist;                  // [S][qcap] its d_t
    double* scal;                   // [S][2]: d, (y_f - mu(x_j)) / d of the current conditioning step
    double* eta;                    // [S] incumbent per sample, lowered by every fantasy
    double *val, *fant;             // [q] winning values, [q][S] fantasy targets
    long long* idx;                 // [q] picks (-1: none)
    unsigned* flg;                  // [q] ROBO_FLAG_* of every pick's values
    int *n_made, *stop;             // picks recorded; a NaN winner ended the selection
    double* trace;                  // q x S x m x 2 transformed, floored (mean, var) every pick was made from, or nullptr
};
struct BatchWork {
    int64_t m;
    int S, n_pad, q;
    char* d_block;
    double* d_trace;
    size_t trace_cap;               // doubles
    char* h_report;                 // pinned copy of the block's tail [val | fant | idx | flg | n_made, stop]: one D2H per call
    size_t rep_off, rep_bytes, off_fant, off_idx, off_flg, off_int;   // the tail in the block; its arrays in the tail (from
                                    // the offsets batch_alloc's BlockLayout returned)
    BatchState st;
};
int batch_alloc(robo_ctx* ctx, int64_t m, int64_t m_pad, int S, int n_pad, int q, BatchWork** out);
void batch_free(BatchWork* w);

// ---- joint Monte-Carlo batch EI (qei.hip) -------------------------------------------------------------------------------------
// what a joint selection keeps on top of a BatchState of its own (whose chist / dhist hold c_t(x) / d_t, whose `fant` slots
// report d_t and whose mean state is never touched); all arrays device memory of one block
constexpr int QEI_MAX_Q = 64, QEI_MAX_K = 1024;
struct QeiState {
    int K;                          // scenarios
    double* z;                      // [K][q] the caller's base samples
    double* b;                      // [S][K] b^k = min(eta_s - par, f^k(picks so far))
    double* acq;                    // q x m every candidate's value at every pick, or nullptr
    double* coef;                   // (q - 1) x S x m c_t(x), or nullptr
    double* best;                   // q x S x K the b^k every pick was made from, or nullptr
};
struct QeiWork {
    int64_t m;
    int S, n_pad, q, K;
    BatchWork* base;                // the picks, the latent moments and the conditioning history (batch.hip's own block)
    char* d_block;                  // z and b, laid out by qei_alloc's BlockLayout (block_layout.h)
    double* d_diag;                 // [acq | coef | best] of a call that asks for them (grows)
    size_t diag_cap;                // doubles
    QeiState qs;
};

// ---- max-value entropy search (mes.hip) ------------------------------------------------------------------------------------
// the state of one call; all arrays device memory of one block, per-sample arrays [S][K] / [S][7]
struct MesState {
    long long m;
    int K, nblk;                    // draws per sample; workgroups of the F pass (128 candidates each)
    double *ystar, *gumbel;         // [S][K] sampled minima; [S][7] w_lo, w_hi, w_1/4, w_1/2, w_3/4, a, b
    double* status;                 // [S] 0 converged, 1 search still open, 2 a NaN moment
    double* u;                      // [S][K] the caller's uniforms
    double* brk;                    // [8]: lower ends [3], upper ends [3] of the quantiles' brackets, the width to reach
    double *bpart, *fpart;          // [nblk][3] bracket partials; [nblk][192] partial F of every grid point
    int* done;                      // the current sample's search has ended: the remaining passes return at once
};
struct MesWork {
    int64_t m;
    int S, K;
    double* d_block;                // [ystar | gumbel | status] (ONE layout entry), u, brk, bpart, fpart, done
    double* d_trace;
    size_t trace_cap;               // doubles
    double* h_stage;               // pinned: [ystar | gumbel | status] of the block's head (one D2H per call), then u
    size_t rep_doubles;
    MesState st;
};
int mes_alloc(int64_t m, int S, int K, MesWork** out);
void mes_free(MesWork* w);

// ---- entropy search's representer chains (represent.hip) ------------------------------------------------------------------
// what the two kernels of a half-step need of ONE chain's model: the posterior of its moving half is formed in that model's
// own candidate handle (the one behind the host-array entry points), exactly as robo_acq_eval forms it
struct RepChain {
    const double* ism;              // [D] inverse square-root metrics of the fitted theta (robo_gp::d_theta)
    double* Xcs;                    // (m_pad, D) the handle's scaled input rows
    const double *mean, *var;       // (m_pad) the handle's transformed mean and floored variance
    double eta;
};
// the state of one call: S chains of k walkers in D dimensions; all arrays device memory of one block
struct RepState {
    int S, k, D, T, normalize;
    long long m_pad;                // rows of a chain's candidate handle (pad rows replicate row 0)
    double a;
    double *pos, *lnp;              // [S][k][D], [S][k]
    double *q, *z;                  // [S][k/2][D], [S][k/2] the pending proposals
    int* outside;                   // [S][k/2] the pending proposal lies outside the box (or is NaN)
    long long* nacc;                // [S][k]
    unsigned* flags;                // [S] ROBO_FLAG_* of every chain's acquisition values
    const double *uz, *ua;          // [S][T][2][k/2] the caller's uniforms, emcee's draw order
    const int* partner;
    const double *lower, *upper;    // [D]
    const RepChain* chain;          // [S]
    double* trace;                  // [S][T][2][k/2][D + 2]: q, lnp(q), code -- or nullptr
};
struct RepWork {
    size_t bytes;                   // of d_block (dev_grow: grows, never shrinks)
    char* d_block;                  // laid out anew by every call (rep_core's BlockLayout)
    double* d_trace;
    size_t trace_cap;               // doubles
};
void rep_free(RepWork* w);

// ---- multi-start MAP optimisation of the hyper-parameters (hyperopt.hip) ------------------------------------------------------
constexpr int HYPER_MAX_STARTS = 64, HYPER_MAX_HISTORY = 16;
// everything a start carries between two launches; all arrays [K], [K][P] or [K][hist][P], device memory of one block
struct HyperState {
    int K, P, D, kind, n, hist, n_iters, prior_kind;
    double mean_c, step0, c1, gtol;
    double prior_par[9];            // mcmc_dev.h PRIOR_PAR
    const double *lower, *upper;    // [P] the box
    double *x, *f, *g, *alpha;      // accepted point, F and G there, current step length
    double *z, *aused;              // pending trial point and the step length it was made with
    double *sh, *yh;                // the (s, y) pairs, oldest first
    int *npairs, *state, *pending;  // pairs held; 0 live / 1 converged / 2 stalled or no direction / 3 dead; the propose kernel's verdict
    int* err;                       // bit 0: a factorisation hand-off timed out
    double* out;                    // [P + 2]: winner's theta, value, index
    double* trace;                  // (n_iters + 1) x K x (2 P + 3), or nullptr
    FitSample* d_sp;                // the batched fit's inputs / outputs (api_fit.hip batch_ensure)
    double* d_ism;
    const double* d_x2max;          // [D] data extents (robo_gp::d_x2max) for gram_needs_direct
    const double *d_out, *d_grad;   // (K x 2) z.z and log det; (K x P) likelihood gradient
    const int* d_fail;
};
// the gradient workspace of a group of samples and the optimiser's state, kept with the GP between calls
struct HyperWork {
    int g_cap, g_npad, g_P;         // samples, n_pad and theta size the gradient workspace was sized for
    double *d_V, *d_A, *d_alpha, *d_part, *d_out;
    int K, P, hist;                 // what d_block was sized for
    char* d_block;                  // [lower | upper | HyperState's arrays]; the four int arrays are ONE layout entry
    double* d_trace;
    size_t trace_cap;               // doubles
};
void hyper_free(HyperWork* w);
int launch_rep_propose(robo_ctx* ctx, const RepState& st, int start, int h, int it);
int launch_rep_accept(robo_ctx* ctx, const RepState& st, int acq_kind, double par, int start, int h, int it);
}  // namespace robo

constexpr int ROBO_AUX_STREAMS = 3;
// robo_ctx_event_record's slots.  Those below EV_GRAM_KERNEL are the caller's; the library records the named ones itself
// (include/robo_hip.h states the same pairs; bench.py and the tools read them by number).  A pair is shared by calls that
// never run inside one another.
enum RoboEventSlot {
    EV_GRAM_KERNEL = 19,      // robo_gp_fit, phase events switched on: 19 -> 21 the gram kernel alone,
    EV_FIT_BEGIN = 20,        //   20 -> 21 the gram phase,
    EV_FIT_GRAM_END = 21,     //   21 -> 22 Cholesky,
    EV_FIT_POTRF_END = 22,    //   22 -> 23 log-likelihood
    EV_FIT_END = 23,
    EV_PREDICT_BEGIN = 24,    // the posterior's last chunk (predict_scaled): 24 -> 25 cross-gram,
    EV_PREDICT_GRAM_END = 25,   // 25 -> 26 triangular solve,
    EV_PREDICT_SOLVE_END = 26,  // 26 -> 27 post
    EV_PREDICT_END = 27,
    EV_GRAD_BEGIN = 28,       // robo_gp_grad_loglik (always): everything after the factorisation; the descent launch of
    EV_GRAD_END = 29,         //   robo_paths_descend (always) and robo_paths_refine_cand
    EV_FOLD_BEGIN = 30,       // what follows the sweeps: KG's envelope kernel and MES's element-wise half (last sample),
    EV_FOLD_END = 31,         //   EHVI's strip kernel, the passes of the path kernel, q-EI's fold kernel of the last pick
    EV_CEI_BEGIN = 32,        // constrained EI's fold kernel
    EV_CEI_END = 33,
    EV_LAST = EV_CEI_END
};
constexpr int ROBO_EVENT_SLOTS = EV_LAST + 1;
constexpr int ROBO_CHAIN_SLOTS = 16;    // chained solves whose time-out words may be in flight between two synchronisations
struct robo_ctx {
    int device;
    hipStream_t stream;
    bool own_stream;
    // side streams of the batched factorisation's sub-batches (potrf.hip), created on first use; fork / join events
    hipStream_t aux[ROBO_AUX_STREAMS];
    hipEvent_t ev_fork, ev_join[ROBO_AUX_STREAMS];
    bool aux_ready;
    // lifetime: handles created on this context (robo_gp, robo_cand, robo_comm, robo_multi) keep it alive.  robo_ctx_destroy
    // marks it `closing`; stream, events and scratch are released when the last such handle is destroyed (api_ctx.hip
    // ctx_retain / ctx_release).  A binding whose garbage collector finalises a context before the objects that live on it
    // (Python's cyclic GC gives no order) therefore cannot make a later robo_gp_destroy touch a dead stream.
    int users;
    bool closing;
    hipEvent_t events[ROBO_EVENT_SLOTS];
    bool phase_events;   // record the internal phase events of robo_gp_fit (robo_ctx_set_phase_events, default off)
    char name[256];
    int num_cu;
    robo::Tuning tune;
    // scratch shared by every call on this context
    double* d_scalars;   // [8]: quad, logdet, ...
    int* d_fail;         // first failing column + 1, or 0
    unsigned* d_prog;    // [2][PROG_STRIDE] progress words of the follower hand-off (potrf.hip), zeroed per factorisation
    double* h_pinned;    // small pinned staging (64 doubles)
    robo::EpWork* ep;    // robo_ep_joint_min's buffers (ep.hip), allocated on first use, grown, never shrunk
    robo::McWork* mc;    // the Monte-Carlo p_min's buffers (igmc.hip), likewise
    // the chained solve (trsm_chain.hip): pinned copies of the time-out words of the launches since the last synchronisation
    // that looked at them (chain_timed_out), how many, and "a launch gave up once: this context stays on the launch path"
    unsigned* h_chain;
    int chain_pending;
    bool chain_off;
};

namespace robo {
// Packed inverse diagonal blocks for the transposed block-row solve (predict.hip): the 36 lower 16x16 sub-blocks x 4
// k-steps of a 128x128 inverse as 64-lane MFMA A-operand fragments, in the order the solve consumes them (row block
// 7 first, column blocks ascending).
constexpr int WP_FRAGS = 144;
constexpr int WP_BLOCK = WP_FRAGS * 64;
__host__ __device__ constexpr int wp_offset(int cb) { return 4 * (36 - (cb + 1) * (cb + 2) / 2); }
}  // namespace robo

struct robo_gp {
    robo_ctx* ctx;
    int kind, dim, n_max;
    int n;          // training points
    int n_pad;      // round_up(n + 1, NB): row n is the augmented (y - mean) row, rest identity
    int n_pad_max;
    bool has_data, fitted;
    unsigned long long fit_gen;   // process-wide serial number of the factor this handle holds (0: none)
    struct robo_cand* host_cand;  // candidate handle behind the host-array entry points, kept between calls of one size
    bool fp32_gram;     // mixed precision: covariance entries evaluated in fp32 (BASELINE config 5)
    robo::CovParams cov;   // kind, dim, amp, blr_a, blr_b of the current theta
    double amp, noise, mean_c;
    double y_mean, y_std;
    double loglik;
    double* d_X;        // (n_max, dim) raw inputs
    double* d_Xs;       // (n_pad_max, dim) inputs scaled by 1/sqrt(metric_d)
    double* d_y;        // (n_max)
    double* d_K;        // (n_pad_max, n_pad_max) gram -> Cholesky factor in place (lower)
    double* d_Linv;     // (n_pad_max / NB) x NB x NB inverses of the diagonal blocks.  With n a multiple of NB the LAST block
                        // (the augmented row alone) is never factored: its inverse slots here and in d_LinvP are ZERO, not
                        // an inverse (robo_gp_set_data clears them); every consumer walks ceil(n / NB) block rows only
    double* d_LinvP;    // the same inverses as packed MFMA A-operand fragments (WP_BLOCK doubles per block, predict.hip)
    double* d_theta;    // inverse sqrt metric (dim) of the current theta
    robo::FitSample* d_sp;   // device copy of the current FitSample
    double x2max[robo::MAX_DIM];   // max_i x_id^2 of the raw training inputs per dimension (robo_gp_set_data)
    double* d_x2max;         // device copy (inside d_theta's block)
    // batch workspace for robo_gp_loglik_batch (lazy, b_cap samples)
    int b_cap, b_npad;
    double *d_bK, *d_bLinv, *d_bXs, *d_bism, *d_bout, *h_bstage;
    robo::FitSample* d_bsp;
    int* d_bfail;
    unsigned* d_bprog;  // [b_cap][PROG_STRIDE] progress words of the batched follower form
    double *d_llpart, *d_bllpart;   // log-likelihood partials of the tail kernel (own factor / batch workspace)
    char* d_bkeep;                  // [b_cap] KeepDst records of robo_gp_fit_batch
    // workspace of robo_gp_grad_loglik (lazy, sized for n_pad_max): W^T, A = alpha alpha^T - K^-1, ...
    double *d_gV, *d_gA, *d_galpha, *d_gpart, *d_gout;
    // explicit inverse factor W = L^-1 for small candidate batches (winv.hip): lazy, rebuilt when the factor changes
    char* d_mcmc;                   // scratch of robo_gp_mcmc_run (one block, lazily grown)
    size_t mcmc_bytes;
    double* d_Winv;                 // (n_pad_max, n_pad_max) row-major, lower block triangle valid
    unsigned long long winv_gen;    // fit_gen the inverse was built for (0: none)
    // unit tables of the triangular product for winv_nbk block rows, one per contraction-chunk depth (the batch depth, half
    // and a quarter of it: small batches take shallower units -- more of them, shorter critical path)
    int* d_wunits[3];               // int4 per unit
    int* d_wprefix[3];              // first canonical unit of every block row (winv_nbk + 1 entries)
    int winv_units[3], winv_kc[3];
    int winv_nbk;
    double diag_min, diag_max;      // extreme diagonal entries of L over the training rows (0, 0: unknown)
    double winv_cond;               // cond_inf(L) = |L|_inf |W|_inf of the factor W was built for (winv_gen); 0: unknown
    double* d_wnorm;                // [2]: |L|_inf, |W|_inf (bit patterns, atomicMax)
    double* h_wnorm;                // pinned copy of the two norms (written by an asynchronous copy behind the build)
    unsigned long long winv_launched;   // fit_gen whose W build has been LAUNCHED (robo_gp_prefetch_inverse) but not yet read
    robo::RefineWork* refine;       // state + solve workspace of robo_acq_refine_* (refine.hip), kept between calls of one (K, D)
    robo::BatchWork* batch;         // state of robo_acq_batch_* (batch.hip), kept between calls of one (m, S)
    robo::QeiWork* qei;             // state of robo_qei_batch_* (qei.hip), kept between calls of one (m, S, q, K)
    robo::MesWork* mes;             // state of robo_mes_eval_* (mes.hip), kept between calls of one (m, S, K)
    robo::RepWork* rep;             // state of robo_rep_sample* (represent.hip), kept with gps[0] between calls
    robo::HyperWork* hyper;         // workspace of robo_gp_grad_loglik_batch / robo_gp_optimize_hypers (hyperopt.hip)
    // the acquisition screen (screen.hip), lazy: [scratch (n_pad_max) | alpha = L^-T z (n_pad_max) | sum_j |alpha_j| sqrt(k_jj),
    // then, for the kinds and D the dot-form bounds kernel takes, its per-fit inputs (screen.hip "The dot form")]
    double* d_alpha;
    double dot_extent;              // sum_d max_j (x_jd - centre_d)^2 of the scaled training rows alpha was computed for
    double dot_alpha_sum;           // sum_j |alpha_j| of the same fit (the lean finish's rule)
    double int_step, int_eps;       // the integer form's grid step h and its covariance error in units of amp (0: no extent, no grid)
    unsigned long long alpha_gen;   // fit_gen alpha was computed for (0: none)
    unsigned long long screen_gen;  // fit_gen the back-off below belongs to
    int screen_skip, screen_backoff;   // eligible calls still to pass unscreened after a failed screen; length of the next pause
    int single_skip, single_backoff;   // the same pair for the screen's single-precision first stage alone (same screen_gen)
};

struct robo_cand {
    robo_ctx* ctx;
    int dim;
    int64_t m;          // candidates
    int64_t m_pad;      // round_up(m, NB)
    double* d_Xc;       // (m_pad, dim) raw candidates (pad rows replicate row 0)
    double* d_Xcs;      // (m_pad, dim) scaled for the GP being evaluated
    double* d_V;        // (chunk, ldv) cross-gram -> L^-1 k_* in place
    int64_t chunk;      // candidates per workspace pass (multiple of NB)
    const char* solve_kernel;   // name of the kernel that ran the last posterior's solve (diagnostics: bench labels)
    int ldv;            // n_pad the workspace was sized for
    size_t v_bytes;
    const robo_gp* solved_gp;        // d_V holds L^-1 k_* of ALL the points for this factor (entropy search keeps
    unsigned long long solved_gen;   // the representer points' solve across compute() calls); 0 = not valid
    double* d_q;        // (m_pad) sum_n V^2
    double* d_mu;       // (m_pad) V . z
    double* d_mean;     // (m_pad) transformed mean
    double* d_var;      // (m_pad) transformed, floored variance
    double* d_acq;      // (m_pad)
    double* d_acq_sum;  // (m_pad) marginal accumulator
    // entropy search (lazy): cross-covariances with the representer points, quadratic-form
    // features / outputs, EP tensors
    double *d_S, *d_F, *d_Q, *d_G, *d_igc;
    size_t f_cap, q_cap, g_cap;
    double* d_kg;       // knowledge gradient (lazy, grows): [S x 64 discretisation means | S x m x (nb + 2) trace]; the expected
                        // hypervolume improvement's [front (4096 x 2) | m x 4 trace] (api_ehvi.hip); constrained EI's trace
                        // (m x (2 (C + 1) + 2)) or, in the moments form, the constraints' [means (C x m) | vars (C x m)]
    size_t kg_cap;
    double* h_igkey;    // host copy of the EP state whose device form d_G / d_igc hold (compared in full before an upload
    size_t igkey_len;   // is skipped: compute() is called many times per update(), information_gain.py:87-125 / :153-167)
    double* d_mu_all;   // (s_cap, m_pad) per-sample means/variances for the GP-MCMC mixture (lazy)
    double* d_var_all;
    int s_cap;
    // explicit-inverse path (winv.hip), lazy: cross-gram K_* (chunk x n_pad), per-unit product tiles, per-block-row
    // partial sums of |v|^2 and v.z
    double *d_Ks, *d_P, *d_qpart;
    size_t ks_bytes, p_bytes, qpart_bytes;
    double* d_part_val; // per-block argmax partials
    long long* d_part_idx;
    unsigned* d_flags;
    int n_part;
    // the acquisition screen (screen.hip), lazy: bounds (m_pad each), survivor counts / offsets per 256 candidates, the
    // survivors' original indices, and the sub-handle that holds their scaled rows and runs their exact solve
    double *d_scr_up, *d_scr_lo;
    int* d_scr_cnt;                 // [n_part + 1] counts -> exclusive offsets, total last
    long long* d_scr_map;           // [scr_sub's capacity]
    struct robo_cand* scr_sub;      // owned; m / m_pad / n_part are set per call to the survivors at hand
    robo::RefineWork* scr_probe;    // the selection state of the probe (refine.hip's top-K), lazy
    int64_t scr_cap;                // rows scr_sub was allocated for
    int64_t scr_n, scr_kept;        // robo_cand_last_screen: candidates screened, survivors
    int scr_outcome;
    const char* scr_bounds_kernel;  // name of the kernel that ran the last bounds pass on this handle (diagnostics: tests)
    int scr_finish;                 // ... and its finish: ROBO_SCREEN_FINISH_* (robo_cand_last_screen_finish)
    int scr_first_stage;            // robo_cand_last_screen_first: 0 no first stage, 1 it decided the call, 2 the fp64 pass followed
    int64_t scr_first_kept;         // ... and its survivor count
    int scr_int;                    // robo_cand_last_screen_form: 1 the last bounds pass took its squared distances from the int8 products
    double scr_int_step;            // ... on this grid step (0 otherwise)
    bool scr_tail_fused;            // the last argmax-only call ran its survivors' tail as acq_tail_kernel (same accessor)
    // the chained solve (trsm_chain.hip), lazy, grows: [ticket | time-out | progress words] zeroed per launch, then the
    // per-(tile, block row) partial sums
    char* d_chain;
    size_t chain_bytes;
    bool defer_post;                // predict_scaled leaves the output transform to the caller's next launch (the screen's fused tail)
    bool best_reported;             // (max, argmax, flags) are in the context's pinned block already: acq_read_back launches no report
    size_t chain_cleared;           // bytes at d_chain's head that a kernel queued on the stream has zeroed for the NEXT chained
                                    // launch (the screen's gather); 0: none, launch_predict_chain runs its memset
};

namespace robo {
// The library's own event slots (24 and above) are recorded for every batch above 16 384 rows.  Small batches are
// latency-bound and an event packet costs microseconds: for them, and for the fit (k = nullptr), only when the phase
// events are switched on (robo_ctx_set_phase_events).
inline bool phase_events_on(const robo_ctx* c, const robo_cand* k) { return c->phase_events || (k && k->m_pad > 16384); }
inline int record_phase(robo_ctx* c, int slot) {
    ROBO_HIP_CHECK(hipEventRecord(c->events[slot], c->stream));
    return ROBO_OK;
}
}  // namespace robo

// ---- launchers implemented in the .hip files (all asynchronous on ctx->stream) ------------
namespace robo {
int launch_scale_inputs(robo_ctx* ctx, const double* d_in, double* d_out, const double* d_inv_sqrt_metric,
                        int64_t rows_real, int64_t rows_pad, int dim, int S = 1, size_t out_stride = 0,
                        size_t ism_stride = 0, unsigned long long* d_word = nullptr, unsigned long long word_value = 0);
// the fit pipeline on S matrices at once (S = 1: the GP's own buffers)
struct FitBuffers {
    double* K; size_t k_stride;          // (n_pad x n_pad) per sample
    double* Linv; size_t linv_stride;    // (n_pad/128 x 128 x 128) per sample
    const double* Xs; size_t xs_stride;  // (n_pad x dim) per sample
    const FitSample* sp;                 // [S]
    int* fail;                           // [S]
    unsigned* prog;                      // [S][PROG_STRIDE] progress words (single-theta fits), or nullptr
    double* out;                         // [S][2]: z.z, 2 sum log diag
    double* ll_part;                     // [S][n_pad/128][4] per block: z.z and sum log L_ii shares, min / max L_ii
    double* LinvP;                       // packed inverse fragments of the GP's own factor, or nullptr (batch workspace)
    double* host_out;                    // pinned host [S][5]: z.z, 2 sum log diag, failure flag, min / max L_ii -- or nullptr
    bool want_inverse;                   // false: log-likelihood only (no explicit inverse blocks, no fragments)
    bool skip_tail;                      // the caller reduces the likelihood terms itself (mcmc.hip mcmc_tail_kernel)
    // launch_gram: a sample of this launch may carry FitSample::direct, so the kernel with both fp64 tiles is launched.  A
    // caller that formed every theta on the host and found none clears it and gets the dot tile's kernel alone.
    bool gram_mixed = true;
    int S;
};
int launch_scale_inputs_theta(robo_ctx* ctx, const double* d_in, double* d_out, const ThetaArgs& ta, int64_t rows_real,
                              int64_t rows_pad, int dim, double* d_ism_out, FitSample* d_sp_out);
// destination of one sample of a batched fit that keeps its factors (fit_keep.hip batch_keep_kernel)
struct KeepDst {
    double *K, *Linv, *LinvP, *Xs, *theta;
    double *X, *y;            // nullptr for gps[0] (owns the training data already)
    FitSample* sp;
    int ok;
};
int launch_batch_keep(robo_gp* g0, const KeepDst* d_dst, int ns);
int launch_gram(robo_gp* gp, const FitBuffers& fb, hipStream_t stream = nullptr, int s0 = 0, int ns = -1);
// the device-resident hyper-parameter chain (mcmc.hip): everything the two kernels around the batched fit need
struct McmcState {
    int k, P, D, kind, n, n_steps, ns_eval, prior_kind;
    double a, mean_c;
    double prior_par[9];            // mcmc_dev.h PRIOR_PAR
    double *d_pos, *d_lnp, *d_q, *d_z, *d_prior;      // (k x P), (k), (k/2 x P), (k/2), (k/2)
    long long* d_nacc;                                // (k)
    int *d_it, *d_err;
    const double *d_uz, *d_ua;                        // (n_steps x 2 x k/2) each, emcee's draw order
    const int* d_partner;
    double *d_chain, *d_lnprob;                       // (k x n_steps x P), (k x n_steps); nullable
    FitSample* d_sp;                                  // the batched fit's inputs / outputs (api_fit.hip batch_ensure)
    double* d_ism;
    const double* d_x2max;                            // [D] data extents (robo_gp::d_x2max) for gram_needs_direct
    const double* d_out;
    const int* d_fail;
};
int launch_mcmc_propose_scale(robo_ctx* ctx, const McmcState& st, int start, int first, int h, int it, const double* d_X,
                              double* d_Xs, int64_t rows_real, int64_t rows_pad, size_t xs_stride);
int launch_mcmc_accept(robo_ctx* ctx, const McmcState& st, int start, int first, int h, int it);
int launch_mcmc_tail(robo_ctx* ctx, const McmcState& st, int start, int first, int h, int it, const double* d_K, size_t k_stride,
                     int ld, int nbf, const int* d_fail);
int launch_mcmc_block_step(robo_gp* gp, const McmcState& st, int start, int first, int h, int it);
// with_gram: the gram matrices are built here too, every sub-batch's on the stream its factorisation runs on
int launch_potrf(robo_gp* gp, const FitBuffers& fb, bool with_gram = false);
int launch_diag_timeline(robo_gp* gp, long long* d_stamps);
int launch_cross_gram(robo_gp* gp, robo_cand* cand, int64_t c0, int64_t cn, double* d_out = nullptr);
// posterior of a chunk through W = L^-1 (winv.hip): fills cand->d_q / d_mu (and d_V when store_v)
int winv_ensure(robo_gp* gp);
int winv_launch(robo_gp* gp);
int launch_per_cost(robo_ctx* ctx, double* d_dh, const double* d_log_cost, double overhead, int64_t m);
int launch_predict_winv(robo_gp* gp, robo_cand* cand, int64_t c0, int64_t cn, bool store_v);
// rows already in memory (the pseudo-rows of the gradient refinement): the buffer to fill, then V = rows W^T into cand->d_V
// with q / mu, in the one form whose rounding does not depend on the row count
int winv_rows_buffer(robo_gp* gp, robo_cand* cand, int64_t rows, double** out);
int launch_winv_rows(robo_gp* gp, robo_cand* cand, int64_t rows);
int launch_trsm(robo_gp* gp, robo_cand* cand, int64_t c0, int64_t cn);
int launch_predict_fused(robo_gp* gp, robo_cand* cand, int64_t c0, int64_t cn);
// trsm_chain.hip: the small-batch block-row solve of a chunk in one launch; whether a chunk takes it; the look at the time-out
// words after a synchronisation of the stream (true: a launch gave up -- the caller repeats its call, which runs the launches)
bool chain_wanted(const robo_gp* gp, int64_t cn);
int launch_predict_chain(robo_gp* gp, robo_cand* cand, int64_t c0, int64_t cn);
int chain_state_ensure(const robo_gp* gp, robo_cand* cand, int64_t cn, size_t* state_bytes_out);
bool chain_timed_out(robo_ctx* ctx);
int launch_pack_linv(robo_gp* gp);
int launch_grad_loglik(robo_gp* gp, double* d_V, double* d_A, double* d_alpha, double* d_part, double* d_out,
                       double* h_out);
int launch_triinv(robo_gp* gp, double* d_W, double* d_V);   // W = L^-1 (and V = W^T) of the current factor
// gradient.hip, S samples per launch: the factors of a batched fit (launch_potrf with want_inverse) -> out (S x P)
struct GradBatch {
    const double* K; size_t k_stride;        // the batched fit's factors, inverse diagonal blocks, scaled inputs and samples
    const double* Linv; size_t linv_stride;
    const double* Xs; size_t xs_stride;
    const FitSample* sp;
    double *V, *A;                           // S x (n_pad x n_pad) each; A doubles as W during the inversion
    double *alpha, *part, *out;              // S x n_pad, S x P x tiles64, S x P
    int S;
};
int launch_grad_loglik_batch(robo_gp* gp, const GradBatch& gb);
// hyperopt.hip: the trial points of all starts (direction, projection, FitSample, scaled inputs); the accept test behind
// the batched fit and gradient; the winner
int launch_hyper_propose(robo_ctx* ctx, const HyperState& st, int t, const double* d_X, double* d_Xs, int64_t rows_real,
                         int64_t rows_pad, size_t xs_stride);
int launch_hyper_accept(robo_ctx* ctx, const HyperState& st, int t);
int launch_hyper_result(robo_ctx* ctx, const HyperState& st);
int launch_post(robo_gp* gp, robo_cand* cand, int64_t c0, int64_t cn);
int launch_cross_grad(robo_gp* gp, const double* d_Xcs, double* d_V, int64_t c_first, int64_t c_count, int64_t rows_pad);
int launch_predgrad_post(robo_gp* gp, const double* d_V, const double* d_q, const double* d_mu, const double* d_Xcs,
                         int64_t c_first, int64_t c_count, double* d_mean, double* d_var, double* d_dmean,
                         double* d_dvar);
// refine.hip: top-K of d_vals (m) -> starts gathered from d_Xc; one value-and-gradient + step launch; the winner
int launch_refine_select(robo_ctx* ctx, const RefineState& st, const double* d_vals, int64_t m, const double* d_Xc,
                         double step0);
int launch_refine_eval(robo_gp* gp, const RefineState& st, const robo_cand* ws, int acq_kind, double par, double eta, int s,
                       int S, int t, int T);
int launch_refine_result(robo_ctx* ctx, const RefineState& st, unsigned* d_cand_flags, bool sweep_only);
// state + pseudo-row workspace for K starts in D dimensions, kept with g between calls of one (K, D)
int refine_ensure(robo_gp* g, int K, int D, RefineWork** out);
// cei_refine.hip: the epilogue of one GP of the constrained refinement at the K trial points.  A constraint (threshold thr)
// adds log Phi(z) and its gradient to the running L / dL in st.fy / st.gy (first: starts them); the objective (objective =
// true, always the last launch of a trial) forms its own factor unless has_eta = 0.  last: combine, decide, next trial.
struct CeiRefineStep {
    bool objective, first, last;
    double thr;
    int C, kind, has_eta;
    double par, eta;
};
int launch_cei_refine_eval(robo_gp* gp, const RefineState& st, const robo_cand* ws, const CeiRefineStep& step, int t, int T);
// batch.hip: outputs to "no pick"; a sample's latent moments after its posterior; the reduction's winner -> pick j; one
// conditioning step (k_*(x_j), beta, the pass over the candidates) of sample s for pick j >= 1
int launch_batch_reset(robo_ctx* ctx, const BatchState& st);
int launch_batch_init(robo_gp* gp, const BatchState& st, const robo_cand* cand, int s, double eta);
int launch_batch_record(robo_ctx* ctx, const BatchState& st, const robo_cand* cand, int j, bool take_flags);
int launch_batch_condition(robo_gp* gp, const BatchState& st, const robo_cand* cand, int s, int j, int acq_kind, double par,
                           int fantasy_kind, double liar);
int launch_acq(robo_ctx* ctx, robo_cand* cand, int acq_kind, double par, double eta, bool accumulate, bool first);
int launch_argmax(robo_cand* cand, const double* d_vals, double scale);
int launch_report_best(robo_cand* cand, double* h_pinned);
int launch_acq_tail(robo_gp* gp, robo_cand* s, int acq_kind, double par, double eta, const long long* d_map, robo_cand* k,
                    double* h_report);
// batch.hip: v = L^-1 w (w is consumed), then beta = L^-T v for ONE right-hand side by forward / backward block rows with
// the fit's inverted diagonal blocks (v is consumed)
int launch_fwd_rows(robo_gp* gp, double* d_w, double* d_v, const int* d_stop);                // *d_stop != 0: no-op
int launch_bwd_rows(robo_gp* gp, double* d_v, double* d_beta, const int* d_stop = nullptr);   // *d_stop != 0: no-op
int launch_cov(robo_gp* gp, robo_cand* cand, double* d_cov);
int launch_mixture(robo_cand* cand, int S);
// clip: floored at DBL_EPSILON as the reference's predict(full_cov=True) (entropy search); false: signed (kg.hip)
int launch_cross_cov(robo_gp* gp, robo_cand* cand, robo_cand* rep, int64_t c0, int64_t cn, double* d_S, bool clip = true);
// kg.hip: the knowledge gradient of candidates c < m from their signed covariance rows d_S (m x NB), d_var, d_mean and the
// nb discretisation means; first: acq_sum[c] = KG, else acq_sum[c] += KG; d_trace (m x (nb + 2)) nullable
int launch_kg(robo_ctx* ctx, const double* d_S, const double* d_var, const double* d_mean, const double* d_disc, int64_t m,
              int nb, double sn2, int include_self, bool first, double* d_acq_sum, unsigned* d_flags, double* d_trace);
// ehvi.hip: the two-objective expected hypervolume improvement of candidates c < m from their four moments over the sorted
// front d_front (P x 2) and the reference point into d_out; d_trace (m x 4: mean1, var1, mean2, var2) nullable
int launch_ehvi(robo_ctx* ctx, const double* d_mean1, const double* d_var1, const double* d_mean2, const double* d_var2,
                const double* d_front, int P, double r1, double r2, int64_t m, double* d_out, unsigned* d_flags,
                double* d_trace);
// cei.hip: EI weighted by the probability of feasibility of candidates c < m from the objective's moments and the C
// constraints' (row k at d_means / d_vars + k * stride) into d_out; the thresholds travel as a kernel argument;
// d_trace (m x (2 (C + 1) + 2): the moments, L, the objective factor) nullable
struct CeiThresholds {
    double t[ROBO_CEI_MAX_CONSTRAINTS];
};
int launch_cei(robo_ctx* ctx, const double* d_mean0, const double* d_var0, const double* d_means, const double* d_vars,
               int64_t stride, int C, const CeiThresholds& th, int kind, double par, double eta, int has_eta, int64_t m,
               double* d_out, unsigned* d_flags, double* d_trace);
int launch_ig_dh(robo_ctx* ctx, const double* d_S, const double* d_var, double* d_F, double* d_Q, const double* d_G,
                 const double* d_consts, int64_t c0, int64_t cn, int64_t m, int nb, int npts, int kf, double sn2,
                 double H, double* d_out);
// igmc.hip: Monte-Carlo information gain of m candidates whose cross-covariances s (m, lds) and variances v (m) are on
// the device, into d_gain (asynchronous); d_counts / d_jit nullable; d_flags nullable (ROBO_FLAG_NOT_FACTORED)
int mc_eval_gains(robo_ctx* c, int64_t m, int nb, int np, int nf, double sn2, const double* d_s, int lds,
                  const double* d_v, const double* Mb, const double* Vb, const double* logP, const double* lmb,
                  const double* W, const double* z, double* d_gain, int* d_counts, double* d_jit, unsigned* d_flags);
int launch_random_candidates(robo_ctx* ctx, double* d_out, int64_t m_pad, int dim, uint64_t seed, int64_t n_uniform,
                             const double* d_loc, const double* d_scale);
int launch_uniform(robo_ctx* ctx, double* d_out, int64_t m, int64_t m_pad, int dim, uint64_t seed);
int launch_sobol(robo_ctx* ctx, double* d_out, int64_t m, int64_t m_pad, int dim, const unsigned long long* d_sv,
                 const unsigned long long* d_shift, int bits, uint64_t first);
int launch_mfma_selftest(robo_ctx* ctx, double* out_err);
int launch_cov_rows_probe(robo_ctx* ctx, const CovParams& cp, const double* h_xi, const double* h_xj, long long n,
                          double* h_out);
int launch_stretch_probe(robo_ctx* ctx, const double* h_c, const double* h_s, const double* h_u, double a, int P, int n,
                         double* h_z, double* h_q, double* h_d);
int launch_gemm_microbench(robo_ctx* ctx, int variant, int wgs, int K, int reps, double* out_tflops);
int launch_clock_sampler(robo_ctx* ctx, int window_us);
int collect_clock_sampler(double* out3);
int launch_mfma_microbench(robo_ctx* ctx, int iters, double* out_tflops, double* out_cycles_per_mfma,
                           double* out_shader_mhz, double* out_chain);
}  // namespace robo
