// The small-batch block-row substitution (predict.hip trsm_step_small_kernel, one launch per block row) as ONE launch whose
// block rows hand their result tiles to each other.
//
// Block row i of  V = L^-1 K_*^T  depends on block row j < i only through the 128 x 16 tile v_j.  The launch-per-row form
// serialises everything else behind it as well: the cross-covariance tile of row i, the loads of L[i][0 .. i-1] and all the
// updates  acc_i -= L[i][j] v_j  with j < i - 1 wait for the launch of row i, and that launch streams the whole block row
// of L (up to 4 MB) through the one CU a 16-candidate tile occupies.  Here one workgroup owns (candidate tile, block row i):
// it generates its cross tile at once, applies every v_j as soon as tile j's progress word is up (right-looking: ascending
// j), then runs the unchanged tail of the step -- the product with the packed inverse diagonal block, the store of v_i and
// the partial |v|^2, v.z sums -- and publishes v_i.  What remains serial per tile is a chain of nbk hand-offs, each behind
// one 128-wide update and one 128 x 128 product, and the block rows of L are read by nbk CUs at once.
//
// Same bits as the launches: every accumulator receives the updates of block column j in ascending j and, inside one, its
// MFMAs in ascending k with the operand roles and the negation of gemm_s (MFMA_ORDER below); the tail is the step kernel's;
// q and mu are summed from per-block-row slots in ascending i starting from slot 0, which is the order in which the launches
// assign (i == 0) and add (i > 0).
//
// Ticket: a workgroup does not use blockIdx.  It takes the next ticket t of a counter and works on tile t / nbk, block row
// t % nbk, and it waits only for lower tickets of its own tile.  The lowest unfinished ticket therefore never waits for an
// unfinished one, whatever order the workgroups are dispatched in and however many of them are resident at a time: the
// launch terminates.  (The interpreter runs one workgroup at a time, i.e. in ticket order: nothing ever waits there.)
//
// Hand-off (common.h): v_i and the (sq, sz) slots are stored write-through (st_agent), every storing wave drains, the
// workgroup meets at its barrier, one lane stores the progress word; the consumer polls that word with one lane (s_sleep
// between polls) and reads v_j and the slots ONLY with L1-bypassing agent loads (ld_agent) -- never through tile_load_regs,
// whose plain loads of a const __restrict__ pointer may be served from a stale L1 line or the scalar cache.  L, LinvP, z and
// the inputs belong to the fit: plain loads.
// Every spin is bounded.  A workgroup that gives up raises the time-out word (atomicMax: a later store cannot clear it) and
// returns without storing anything; the workgroups that depend on it give up in turn.  The host looks at the word at the
// synchronisation the call ends in anyway, repeats the solve by launches and keeps the context off this path (chain_timed_out).
#include "api_internal.h"
#include "trsm_small.h"

namespace robo {

constexpr int CHAIN_HDR = 4;            // unsigned words ahead of the progress words: ticket, time-out, two of padding
constexpr int CHAIN_SLOT = 32;          // doubles per (tile, block row) slot: sq of the 16 candidates, then sz
template <int DK> constexpr int chain_stage() { return DK * NB * LDS_LD; }      // DK k-tiles of L[i][j]
constexpr int CHAIN_VLD = NB + 2;       // leading dimension of the v_j image [16 candidates][128]
template <int DK> constexpr int chain_smem_doubles() {   // two staging stages | v_j   (the tail's two images fit in the stages)
    return 2 * chain_stage<DK>() + 16 * CHAIN_VLD;
}

// DK = k-tiles of 16 per staging stage, as in gemm_s: 2 while one workgroup per CU covers the grid (75 + 17 KB of LDS), 1 beyond
template <int KIND, int DK>
__global__ __launch_bounds__(256) void trsm_chain_kernel(const double* __restrict__ Xcs, const double* __restrict__ Xs,
                                                         double* V, int ldv, const double* __restrict__ L, int ld,
                                                         const double* __restrict__ LinvP, int nbk, int n, double* q,
                                                         double* mu, long long c0, long long m, unsigned* state,
                                                         double* slots, unsigned spin_limit, CovParams cp) {
    constexpr int MB = 1, SA = NB * LDS_LD, STAGE = chain_stage<DK>(), NST = NB / (BK * DK);
    static_assert(2 * STAGE >= 2 * MB * NB * 16 && 2 * STAGE >= 16 * (NB + 2 + 16 * MB + 2), "the stages hold the tile generator's and the tail's images");
    __shared__ double smem[chain_smem_doubles<DK>()];
    __shared__ unsigned s_word;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, nn = lane & 15;
    if (threadIdx.x == 0) s_word = __hip_atomic_fetch_add(state, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const unsigned tk = s_word;
    const int tile = (int)(tk / (unsigned)nbk), i = (int)(tk % (unsigned)nbk);
    const long long cw = c0 + (long long)tile * 16;
    if (cw >= m) {
        // a tile of padding rows only (they replicate row 0): nobody reads its mean, variance, acquisition value or V
        // ("chained solve"), so it is not solved; q and mu get defined values for post_kernel
        if (i == 0 && threadIdx.x < 16) {
            q[cw + threadIdx.x] = 0.0;
            mu[cw + threadIdx.x] = 0.0;
        }
        return;
    }
    unsigned* prog = state + CHAIN_HDR + (size_t)tile * nbk;
    double* slot = slots + (size_t)tile * nbk * CHAIN_SLOT;
    double* Vrow = V + (size_t)tile * 16 * ldv;
    const int n_valid = n - i * NB;
    AccS<MB> acc;
    gen_cross_tile_s<KIND, MB>(cp, Xcs + (size_t)cw * cp.dim, Xs + (size_t)i * NB * cp.dim, n_valid, smem, acc);
    // ---- acc -= L[i][j] v_j for j = 0 .. i - 1, each as soon as v_j is published.  The stages of L run on across the
    // block columns (L needs no hand-off): while the workgroup waits for v_j, the first stage of L[i][j] is in LDS and the
    // second in registers.
    double* sV = smem + 2 * STAGE;
    const double* Lrow = L + (size_t)i * NB * ld;
    const int total = i * NST;
    Tile4 ra[DK];
    if (total > 0) {
#pragma unroll
        for (int u = 0; u < DK; ++u) ra[u] = tile_load_regs<128>(Lrow, ld, u * BK);
#pragma unroll
        for (int u = 0; u < DK; ++u) tile_store_lds<128>(smem + u * SA, ra[u]);
    }
    // MFMA_ORDER: accumulator (rbl, 0) of wave w receives, for j ascending and inside a block column for k ascending in
    // steps of 4,  mfma(a = L[128 i + 32 w + 16 rbl + (lane & 15)][k + (lane >> 4)],  b = -v[candidate lane & 15][k + (lane >> 4)])
    // -- gemm_s's sequence over columns 128 j .. 128 j + 127 with its operand roles and its negation of b; the depth of a
    // staging stage does not enter the arithmetic.
    for (int s = 0; s < total; ++s) {
        const int j = s / NST, st = s % NST;
        const double* cur = smem + (s & 1) * STAGE;
        double* nxt = smem + ((s + 1) & 1) * STAGE;
        const bool more = s + 1 < total;
        if (more) {
#pragma unroll
            for (int u = 0; u < DK; ++u) ra[u] = tile_load_regs<128>(Lrow, ld, ((s + 1) * DK + u) * BK);
        }
        if (st == 0) {
            if (threadIdx.x == 0) {
                unsigned spins = 0, v;
                while ((v = ld_agent_u32(prog + j)) == 0u) {
                    if (spins >= spin_limit) break;
                    ++spins;
                    __builtin_amdgcn_s_sleep(2);
                }
                if (v == 0u) atomicMax(state + 1, tk + 1u);       // gave up: the ticket that did, never cleared by another
                s_word = v;
            }
            __syncthreads();
            if (s_word == 0u) return;                              // (uniform) nothing stored, nothing published
            {   // v_j -> LDS: candidate t / 16, eight consecutive entries, L1-bypassing loads
                const int cand = threadIdx.x >> 4, k8 = (threadIdx.x & 15) * 8;
                const double* src = Vrow + (size_t)cand * ldv + (size_t)j * NB + k8;
                double v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = ld_agent(src + e);
#pragma unroll
                for (int e = 0; e < 8; ++e) sV[cand * CHAIN_VLD + k8 + e] = v[e];
            }
            __syncthreads();
        }
#pragma unroll
        for (int u = 0; u < DK; ++u) {
            const double* pa = cur + u * SA + (wave * 32 + (lane & 15)) * LDS_LD + (lane >> 4);
            const double* pb = sV + (lane & 15) * CHAIN_VLD + (st * DK + u) * BK + (lane >> 4);
#pragma unroll
            for (int kk = 0; kk < BK / 4; ++kk) {
                double a[2];
#pragma unroll
                for (int rbl = 0; rbl < 2; ++rbl) a[rbl] = pa[rbl * 16 * LDS_LD + kk * 4];
                const double b = -pb[kk * 4];
#pragma unroll
                for (int rbl = 0; rbl < 2; ++rbl) acc.t[rbl][0] = mfma_f64(a[rbl], b, acc.t[rbl][0]);
            }
        }
        if (more) {
#pragma unroll
            for (int u = 0; u < DK; ++u) tile_store_lds<128>(nxt + u * SA, ra[u]);
        }
        __syncthreads();
    }
    // ---- the tail of trsm_step_small_kernel (MB = 1); v_i and the partial sums leave write-through
    double* sT = smem;
    double* sO = smem + MB * NB * 16;
#pragma unroll
    for (int rbl = 0; rbl < 2; ++rbl)
#pragma unroll
        for (int r = 0; r < 4; ++r) sT[(wave * 32 + rbl * 16 + g + 4 * r) * 16 + nn] = acc.t[rbl][0][r];
    __syncthreads();
    const double* wp = LinvP + (size_t)i * WP_BLOCK + lane;
    const double* z = L + (size_t)n * ld + (size_t)i * NB;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int cb = half == 0 ? wave : 7 - wave;
        v4d o = v4d{0.0, 0.0, 0.0, 0.0};
        const double* wf = wp + (size_t)wp_offset(cb) * 64;
        for (int jb = 0; jb <= cb; ++jb) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) o = mfma_f64(wf[(4 * jb + kk) * 64], sT[(16 * jb + 4 * kk + g) * 16 + nn], o);
        }
        const int r0 = 16 * cb + 4 * g;
        double* dst = Vrow + (size_t)nn * ldv + (size_t)i * NB + r0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double v = r0 + r < n_valid ? o[r] : 0.0;
            sO[(r0 + r) * 16 + nn] = v;
            st_agent(dst + r, v);
        }
    }
    __syncthreads();
    double sq = 0.0, sz = 0.0;
    if (wave < MB) {
#pragma unroll
        for (int cbi = 0; cbi < 8; ++cbi) {
            const int r0 = 16 * (7 - cbi) + 4 * g;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double v = sO[(r0 + r) * 16 + nn];
                const double zc = r0 + r < n_valid ? z[r0 + r] : 0.0;
                sq = fma(v, v, sq);
                sz = fma(v, zc, sz);
            }
        }
        sq += __shfl_xor(sq, 16);
        sz += __shfl_xor(sz, 16);
        sq += __shfl_xor(sq, 32);
        sz += __shfl_xor(sz, 32);
    }
    if (i + 1 < nbk) {
        if (wave < MB && g == 0) {
            st_agent(slot + (size_t)i * CHAIN_SLOT + nn, sq);
            st_agent(slot + (size_t)i * CHAIN_SLOT + 16 + nn, sz);
        }
        drain_vmem();                      // every storing wave: v_i and the slot have left the CU
        __syncthreads();
        // spin_limit == 0 is the tests' time-out drill: nothing is published, so the first consumer's first poll fails
        if (threadIdx.x == 0 && spin_limit != 0u) st_agent_u32(prog + i, 1u);
        return;
    }
    // ---- the last block row: its own hand-offs imply every earlier one, slots included.  q and mu as the launches leave
    // them: slot 0 assigned, the others added in ascending i.
    if (wave < MB && g == 0) {
        double tq = ld_agent(slot + nn), tz = ld_agent(slot + 16 + nn);
        for (int r = 1; r < i; ++r) {
            tq += ld_agent(slot + (size_t)r * CHAIN_SLOT + nn);
            tz += ld_agent(slot + (size_t)r * CHAIN_SLOT + 16 + nn);
        }
        tq += sq;
        tz += sz;
        q[cw + nn] = tq;
        mu[cw + nn] = tz;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// the batch takes the chained form (the caller has already ruled out the explicit inverse, fp32 entries and the stepwise form)
bool chain_wanted(const robo_gp* gp, int64_t cn) {
    const robo_ctx* c = gp->ctx;
    const Tuning& t = c->tune;
    if (t.trsm_chain == 0 || c->chain_off || c->chain_pending >= ROBO_CHAIN_SLOTS) return false;
    const int64_t nbk = (gp->n + NB - 1) / NB;
    if (cn > t.trsm_small_max || nbk < 2) return false;     // one block row has no chain
    if (t.trsm_chain > 0) return true;
    // automatic: from three block rows on (two launches against one launch, its memset and the copy of its time-out word were
    // not measured, and tests/test_acq_screen.py pins the step kernel's name for survivors at N = 256), while the grid stays
    // within the measured bound (NOTES.md: faster up to 4 workgroups per CU at N = 1024 and N = 4096, slower at 16 / 64)
    if (nbk < 3) return false;
    return cn / 16 * nbk <= (int64_t)t.trsm_chain_max_wg * c->num_cu;
}

int launch_predict_chain(robo_gp* gp, robo_cand* cand, int64_t c0, int64_t cn) {
    robo_ctx* c = gp->ctx;
    const int nbk = (gp->n + NB - 1) / NB;
    const int64_t tiles = cn / 16, wgs = tiles * nbk;
    // [ticket | time-out | pad | pad | progress words], padded to 16 bytes and zeroed before every launch; the slots behind it
    const size_t state_bytes = (size_t)round_up64((CHAIN_HDR + wgs) * (int64_t)sizeof(unsigned), 16);
    const size_t slot_off = (size_t)round_up64((int64_t)state_bytes, 256);
    const size_t need = slot_off + (size_t)wgs * CHAIN_SLOT * sizeof(double);
    if (need > cand->chain_bytes) {
        if (cand->d_chain) ROBO_HIP_CHECK(hipFree(cand->d_chain));
        cand->d_chain = nullptr;
        cand->chain_bytes = 0;
        ROBO_HIP_CHECK(hipMalloc((void**)&cand->d_chain, need));
        cand->chain_bytes = need;
    }
    if (!c->h_chain) ROBO_HIP_CHECK(hipHostMalloc((void**)&c->h_chain, ROBO_CHAIN_SLOTS * sizeof(unsigned), 0));
    unsigned* state = reinterpret_cast<unsigned*>(cand->d_chain);
    double* slots = reinterpret_cast<double*>(cand->d_chain + slot_off);
    const Tuning& tune = c->tune;
    const unsigned spin_limit = tune.trsm_chain_spin_limit >= 0 ? (unsigned)tune.trsm_chain_spin_limit : PROG_SPIN_LIMIT;
    const bool deep = tune.trsm_small_deep >= 0 ? tune.trsm_small_deep != 0 : wgs <= c->num_cu;
    ROBO_HIP_CHECK(hipMemsetAsync(state, 0, state_bytes, c->stream));
    cand->solve_kernel = "trsm_chain_kernel";
#define ROBO_CHAIN_LAUNCH(KIND, DK)                                                                              \
    hipLaunchKernelGGL((trsm_chain_kernel<KIND, DK>), dim3((unsigned)wgs), dim3(256), 0, c->stream,              \
                       (const double*)cand->d_Xcs, (const double*)gp->d_Xs, cand->d_V, gp->n_pad,               \
                       (const double*)gp->d_K, gp->n_pad, (const double*)gp->d_LinvP, nbk, gp->n, cand->d_q,     \
                       cand->d_mu, (long long)c0, (long long)cand->m, state, slots, spin_limit, gp->cov)
#define ROBO_CHAIN_CALL(KIND)                        \
    do {                                             \
        if (deep) ROBO_CHAIN_LAUNCH(KIND, 2);        \
        else ROBO_CHAIN_LAUNCH(KIND, 1);             \
    } while (0)
    if (gp->kind == ROBO_KERNEL_MATERN52_ARD) ROBO_CHAIN_CALL(ROBO_KERNEL_MATERN52_ARD);
    else if (gp->kind == ROBO_KERNEL_RBF_ARD) ROBO_CHAIN_CALL(ROBO_KERNEL_RBF_ARD);
    else ROBO_CHAIN_CALL(ROBO_KERNEL_FABOLAS);
#undef ROBO_CHAIN_CALL
#undef ROBO_CHAIN_LAUNCH
    ROBO_LAUNCH_CHECK();
    // the time-out word rides to pinned memory behind the kernel; the entry point reads it at the synchronisation it ends in
    ROBO_HIP_CHECK(hipMemcpyAsync(c->h_chain + c->chain_pending, state + 1, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    ++c->chain_pending;
    return ROBO_OK;
}

// After a synchronisation of the context's stream: did a chained solve since the last look give up?  Then the context leaves
// the chained form for good (robo_ctx_set_tuning of trsm_chain re-arms it), the message is left for robo_last_error_string,
// and the caller repeats its call, which now runs the launches.
bool chain_timed_out(robo_ctx* c) {
    unsigned worst = 0;
    for (int s = 0; s < c->chain_pending; ++s)
        if (c->h_chain[s] > worst) worst = c->h_chain[s];
    c->chain_pending = 0;
    if (worst == 0) return false;
    c->chain_off = true;
    set_error("trsm_chain_kernel: a hand-off did not arrive within its spin limit (ticket %u gave up); the solve was repeated by "
              "launches and this context no longer uses the chained solve", worst - 1);
    return true;
}

}  // namespace robo
