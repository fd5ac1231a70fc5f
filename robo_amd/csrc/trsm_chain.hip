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
// A link of that chain is: v_{i-1} arrives, the last update, the tail, the store of v_i, its announcement.  Nothing in it
// waits for data of the fit (L, LinvP, z, the inputs: plain loads), which is fetched ahead of the waits:
//  * with the ticket: this wave's 36 fragments of the packed inverse block into registers, the block row's 128 entries of z
//    into an LDS strip, the first stages of L[i][0].  The tail's product loop and the sums read no global memory.
//  * DK = 2 (one workgroup per CU): the WHOLE block column L[i][j], four stages, is on chip before the wait for v_j begins,
//    stages 0 and 1 in the two LDS stages, 2 and 3 in registers, every load complete -- the poll is the only load in flight.
//    The fetch of L[i][j + 1] starts when v_j has been read and stages 0 and 1 applied, under the remaining MFMAs.
//  * DK = 1 (two workgroups per CU) keeps the staging of one stage ahead: a block column is eight stages there, and six of
//    them in registers would take the kernel past 256 registers and its second workgroup off the CU.
//
// Hand-off (common.h), two announcements per block row.  v_i is stored write-through in 16-byte pieces (st_agent2), every
// wave drains, the workgroup meets at its barrier, one lane stores the tile's progress word i.  Only then wave 0 forms the
// (sq, sz) sums -- the next block row does not need them --, stores them write-through in the slot, drains, the barrier
// again, one lane adds 1 to the tile's slot counter.  A consumer polls with one lane (s_sleep between polls): progress word
// j before block column j, and the last block row, whose own hand-offs imply every earlier v but not every earlier slot, the
// counter until it reads nbk - 1.  v_j and the slots are read ONLY with L1-bypassing agent loads (ld_agent2x4, ld_agent) behind
// the barrier the polling lane joins -- never through tile_load_regs, whose plain loads of a const __restrict__ pointer may be
// served from a stale L1 line or the scalar cache.
// State block, zeroed by one hipMemsetAsync before every launch: CHAIN_HDR words (ticket, time-out, padding), then per tile
// chain_tile_words(nbk) words: the nbk progress words and the slot counter.  The slots follow in the same allocation.
// Every spin is bounded.  A workgroup that gives up raises the time-out word (atomicMax: a later store cannot clear it) and
// returns without storing anything; the workgroups that depend on it give up in turn.  The host looks at the word at the
// synchronisation the call ends in anyway, repeats the solve by launches and keeps the context off this path (chain_timed_out).
#include "api_internal.h"
#include "trsm_small.h"

namespace robo {

constexpr int CHAIN_HDR = 4;            // unsigned words ahead of the tiles' words: ticket, time-out, two of padding
// unsigned words per tile behind the header: the nbk progress words ("v_i of this tile is published", 0 / 1), then the
// tile's slot counter (how many of its block rows have published their (sq, sz) slot)
constexpr int chain_tile_words(int nbk) { return nbk + 1; }
constexpr int CHAIN_SLOT = 32;          // doubles per (tile, block row) slot: sq of the 16 candidates, then sz
template <int DK> constexpr int chain_stage() { return DK * NB * LDS_LD; }      // DK k-tiles of L[i][j]
constexpr int CHAIN_VLD = NB + 2;       // leading dimension of the v_j image [16 candidates][128]
template <int DK> constexpr int chain_smem_doubles() {   // two staging stages | v_j | z_i   (the tail's two images fit in the stages)
    return 2 * chain_stage<DK>() + 16 * CHAIN_VLD + NB;
}

// one staging stage of the update: acc -= L[i][j][:, 16 kt .. 16 (kt + DK) - 1] v_j[16 kt ..], see MFMA_ORDER
template <int DK>
__device__ __forceinline__ void chain_update(AccS<1>& acc, const double* cur, const double* sV, int kt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int u = 0; u < DK; ++u) {
        const double* pa = cur + u * NB * LDS_LD + (wave * 32 + (lane & 15)) * LDS_LD + (lane >> 4);
        const double* pb = sV + (lane & 15) * CHAIN_VLD + (kt + u) * BK + (lane >> 4);
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
}

// Thread 0 polls *w (one L1-bypassing load per poll, s_sleep between polls) until it reads `want`, at most spin_limit times;
// everybody learns the outcome behind the barrier.  false (uniform): it gave up and raised the time-out word with its
// ticket (atomicMax: a later store cannot clear it); the workgroup stores nothing more and returns.
__device__ __forceinline__ bool chain_wait(const unsigned* w, unsigned want, unsigned spin_limit, unsigned* state, unsigned tk,
                                           unsigned* s_word) {
    if (threadIdx.x == 0) {
        unsigned spins = 0, v;
        while ((v = ld_agent_u32(w)) != want) {
            if (spins >= spin_limit) break;
            ++spins;
            __builtin_amdgcn_s_sleep(2);
        }
        if (v != want) atomicMax(state + 1, tk + 1u);
        *s_word = v == want ? 1u : 0u;
    }
    __syncthreads();
    return *s_word != 0u;
}

// v_j -> LDS: thread t takes candidate t / 16 and eight consecutive entries, as four 16-byte L1-bypassing loads
__device__ __forceinline__ void chain_load_v(const double* Vrow, int ldv, int j, double* sV) {
    const int cand = threadIdx.x >> 4, k8 = (threadIdx.x & 15) * 8;
    const double* src = Vrow + (size_t)cand * ldv + (size_t)j * NB + k8;
    double2 a, b, c, d;
    ld_agent2x4(src, a, b, c, d);
    double2* dst = reinterpret_cast<double2*>(sV + cand * CHAIN_VLD + k8);
    dst[0] = a;
    dst[1] = b;
    dst[2] = c;
    dst[3] = d;
}

// DK = k-tiles of 16 per staging stage, as in gemm_s: 2 while one workgroup per CU covers the grid (75 + 18 KB of LDS), 1 beyond
template <int KIND, int DK>
__global__ __launch_bounds__(256) void trsm_chain_kernel(const double* __restrict__ Xcs, const double* __restrict__ Xs,
                                                         double* V, int ldv, const double* __restrict__ L, int ld,
                                                         const double* __restrict__ LinvP, int nbk, int n, double* q,
                                                         double* mu, long long c0, long long m, unsigned* state,
                                                         double* slots, unsigned spin_limit, CovParams cp) {
    constexpr int MB = 1, SA = NB * LDS_LD, STAGE = chain_stage<DK>(), NST = NB / (BK * DK);
    // the whole of a block column on chip before its v_j is waited for: two stages in LDS, two in registers.  At DK = 1 a
    // block column is eight stages, and six of them in registers (96) on top of the 72 of the inverse block would take the
    // kernel past 256 registers and its second workgroup off the CU: that instantiation stages one stage ahead
    constexpr bool WHOLE = DK == 2;
    static_assert(!WHOLE || NST == 4, "two stages in LDS and two in registers are a block column");
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
    unsigned* prog = state + CHAIN_HDR + (size_t)tile * chain_tile_words(nbk);
    unsigned* slot_count = prog + nbk;
    double* slot = slots + (size_t)tile * nbk * CHAIN_SLOT;
    double* Vrow = V + (size_t)tile * 16 * ldv;
    const int n_valid = n - i * NB;
    double* sV = smem + 2 * STAGE;
    double* sZ = sV + 16 * CHAIN_VLD;
    const double* Lrow = L + (size_t)i * NB * ld;
    const double* wp = LinvP + (size_t)i * WP_BLOCK + lane;
    const double* z = L + (size_t)n * ld + (size_t)i * NB;
    // ---- what belongs to the fit and is known with the ticket is fetched now, ahead of every wait: this wave's 36
    // fragments of the packed inverse diagonal block (column block `wave` from register 0 upwards, column block 7 - wave from
    // register 35 downwards), the block row's 128 entries of z and the first stages of L[i][0]
    double wreg[36];
    {
        const double* w0 = wp + (size_t)wp_offset(wave) * 64;
        const double* w1 = wp + (size_t)wp_offset(7 - wave) * 64;
        const int n0 = 4 * (wave + 1);
#pragma unroll
        for (int f = 0; f < 36; ++f) wreg[f] = f < n0 ? w0[f * 64] : w1[(35 - f) * 64];
    }
    double zreg = 0.0;
    if (threadIdx.x < NB && (int)threadIdx.x < n_valid) zreg = z[threadIdx.x];
    Tile4 ra[DK], rb[DK];
    if (WHOLE && i > 0) {
#pragma unroll
        for (int u = 0; u < DK; ++u) ra[u] = tile_load_regs<128>(Lrow, ld, u * BK);
#pragma unroll
        for (int u = 0; u < DK; ++u) rb[u] = tile_load_regs<128>(Lrow, ld, (DK + u) * BK);
    }
    AccS<MB> acc;
    gen_cross_tile_s<KIND, MB>(cp, Xcs + (size_t)cw * cp.dim, Xs + (size_t)i * NB * cp.dim, n_valid, smem, acc);
    if (threadIdx.x < NB) sZ[threadIdx.x] = zreg;      // (read behind the tail's barriers)
    // ---- acc -= L[i][j] v_j for j = 0 .. i - 1, each as soon as v_j is published.  L needs no hand-off and runs ahead.
    // MFMA_ORDER: accumulator (rbl, 0) of wave w receives, for j ascending and inside a block column for k ascending in
    // steps of 4,  mfma(a = L[128 i + 32 w + 16 rbl + (lane & 15)][k + (lane >> 4)],  b = -v[candidate lane & 15][k + (lane >> 4)])
    // -- gemm_s's sequence over columns 128 j .. 128 j + 127 with its operand roles and its negation of b; the depth of a
    // staging stage and where a stage waits do not enter the arithmetic.
    if (WHOLE) {
        // Entering iteration j, ra / rb hold (or are receiving) stages 0 and 1 of L[i][j] and both LDS stages are free.
        // They go to LDS, stages 2 and 3 follow into the registers, and only when all of it has arrived does the wait for
        // v_j begin: the poll is the one load in flight, and between its match and the tail nothing waits for memory but
        // v_j itself.  The fetch of L[i][j + 1] starts behind the first two stages' MFMAs, when the registers are free.
        double* b0 = smem;
        double* b1 = smem + STAGE;
        for (int j = 0; j < i; ++j) {
            const int k0 = j * NB;
#pragma unroll
            for (int u = 0; u < DK; ++u) tile_store_lds<128>(b0 + u * SA, ra[u]);
#pragma unroll
            for (int u = 0; u < DK; ++u) tile_store_lds<128>(b1 + u * SA, rb[u]);
#pragma unroll
            for (int u = 0; u < DK; ++u) ra[u] = tile_load_regs<128>(Lrow, ld, k0 + (2 * DK + u) * BK);
#pragma unroll
            for (int u = 0; u < DK; ++u) rb[u] = tile_load_regs<128>(Lrow, ld, k0 + (3 * DK + u) * BK);
            drain_vmem();
            if (!chain_wait(prog + j, 1u, spin_limit, state, tk, &s_word)) return;     // (uniform) nothing stored, nothing published
            chain_load_v(Vrow, ldv, j, sV);
            __syncthreads();
            chain_update<DK>(acc, b0, sV, 0);
            chain_update<DK>(acc, b1, sV, DK);
            __syncthreads();
#pragma unroll
            for (int u = 0; u < DK; ++u) tile_store_lds<128>(b0 + u * SA, ra[u]);
#pragma unroll
            for (int u = 0; u < DK; ++u) tile_store_lds<128>(b1 + u * SA, rb[u]);
            if (j + 1 < i) {
#pragma unroll
                for (int u = 0; u < DK; ++u) ra[u] = tile_load_regs<128>(Lrow, ld, k0 + NB + u * BK);
#pragma unroll
                for (int u = 0; u < DK; ++u) rb[u] = tile_load_regs<128>(Lrow, ld, k0 + NB + (DK + u) * BK);
            }
            __syncthreads();
            chain_update<DK>(acc, b0, sV, 2 * DK);
            chain_update<DK>(acc, b1, sV, 3 * DK);
            __syncthreads();
        }
    } else {
        // one stage ahead: while the workgroup waits for v_j, the first stage of L[i][j] is in LDS and the second in registers
        const int total = i * NST;
        if (total > 0) {
#pragma unroll
            for (int u = 0; u < DK; ++u) ra[u] = tile_load_regs<128>(Lrow, ld, u * BK);
#pragma unroll
            for (int u = 0; u < DK; ++u) tile_store_lds<128>(smem + u * SA, ra[u]);
        }
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
                if (!chain_wait(prog + j, 1u, spin_limit, state, tk, &s_word)) return;
                chain_load_v(Vrow, ldv, j, sV);
                __syncthreads();
            }
            chain_update<DK>(acc, cur, sV, st * DK);
            if (more) {
#pragma unroll
                for (int u = 0; u < DK; ++u) tile_store_lds<128>(nxt + u * SA, ra[u]);
            }
            __syncthreads();
        }
    }
    // ---- the tail of trsm_step_small_kernel (MB = 1), its operands on chip already; v_i leaves write-through in 16-byte pieces
    double* sT = smem;
    double* sO = smem + MB * NB * 16;
#pragma unroll
    for (int rbl = 0; rbl < 2; ++rbl)
#pragma unroll
        for (int r = 0; r < 4; ++r) sT[(wave * 32 + rbl * 16 + g + 4 * r) * 16 + nn] = acc.t[rbl][0][r];
    __syncthreads();
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int cb = half == 0 ? wave : 7 - wave;
        v4d o = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int jb = 0; jb < 8; ++jb) {
            if (jb <= cb) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const double w = half == 0 ? wreg[4 * jb + kk] : wreg[35 - (4 * jb + kk)];
                    o = mfma_f64(w, sT[(16 * jb + 4 * kk + g) * 16 + nn], o);
                }
            }
        }
        const int r0 = 16 * cb + 4 * g;
        double* dst = Vrow + (size_t)nn * ldv + (size_t)i * NB + r0;
        double v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            v[r] = r0 + r < n_valid ? o[r] : 0.0;
            sO[(r0 + r) * 16 + nn] = v[r];
        }
        st_agent2(dst, make_double2(v[0], v[1]));
        st_agent2(dst + 2, make_double2(v[2], v[3]));
    }
    const bool last = i + 1 == nbk;
    // ---- first announcement: v_i.  Every wave has stored its part of it and drains, the barrier, one lane raises the
    // progress word.  (spin_limit == 0 is the tests' time-out drill: nothing is published, neither v_i nor the slot, so the
    // first consumer's first poll fails.)  The sums are nobody's business but the last block row's and come after it.
    drain_vmem();
    __syncthreads();
    if (!last && threadIdx.x == 0 && spin_limit != 0u) st_agent_u32(prog + i, 1u);
    double sq = 0.0, sz = 0.0;
    if (wave < MB) {
#pragma unroll
        for (int cbi = 0; cbi < 8; ++cbi) {
            const int r0 = 16 * (7 - cbi) + 4 * g;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double v = sO[(r0 + r) * 16 + nn];
                const double zc = sZ[r0 + r];
                sq = fma(v, v, sq);
                sz = fma(v, zc, sz);
            }
        }
        sq += __shfl_xor(sq, 16);
        sz += __shfl_xor(sz, 16);
        sq += __shfl_xor(sq, 32);
        sz += __shfl_xor(sz, 32);
    }
    if (!last) {
        // ---- second announcement: the slot, by the same form (write-through, drain, barrier, one lane) on the tile's counter
        if (wave < MB && g == 0) {
            st_agent(slot + (size_t)i * CHAIN_SLOT + nn, sq);
            st_agent(slot + (size_t)i * CHAIN_SLOT + 16 + nn, sz);
        }
        drain_vmem();
        __syncthreads();
        if (threadIdx.x == 0 && spin_limit != 0u) add_agent_u32(slot_count, 1u);
        return;
    }
    // ---- the last block row: q and mu as the launches leave them, slot 0 assigned, the others added in ascending i.  Its
    // hand-offs imply every earlier v, not every earlier slot: it waits until the counter shows all of them.
    if (!chain_wait(slot_count, (unsigned)i, spin_limit, state, tk, &s_word)) return;
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

// the state block of a chained solve of cn candidates on this handle, grown if need be: [ticket | time-out | pad | pad | per
// tile: progress words, slot counter], padded to 16 bytes and zeroed before every launch; the slots behind it
int chain_state_ensure(const robo_gp* gp, robo_cand* cand, int64_t cn, size_t* state_bytes_out) {
    const int nbk = (gp->n + NB - 1) / NB;
    const int64_t tiles = cn / 16, wgs = tiles * nbk;
    const size_t state_bytes = (size_t)round_up64((CHAIN_HDR + tiles * chain_tile_words(nbk)) * (int64_t)sizeof(unsigned), 16);
    const size_t slot_off = (size_t)round_up64((int64_t)state_bytes, 256);
    const size_t need = slot_off + (size_t)wgs * CHAIN_SLOT * sizeof(double);
    if (need > cand->chain_bytes) {
        if (cand->d_chain) ROBO_HIP_CHECK(hipFree(cand->d_chain));
        cand->d_chain = nullptr;
        cand->chain_bytes = 0;
        cand->chain_cleared = 0;
        ROBO_HIP_CHECK(hipMalloc((void**)&cand->d_chain, need));
        cand->chain_bytes = need;
    }
    *state_bytes_out = state_bytes;
    return ROBO_OK;
}

int launch_predict_chain(robo_gp* gp, robo_cand* cand, int64_t c0, int64_t cn) {
    robo_ctx* c = gp->ctx;
    const int nbk = (gp->n + NB - 1) / NB;
    const int64_t tiles = cn / 16, wgs = tiles * nbk;
    size_t state_bytes = 0;
    ROBO_TRY(chain_state_ensure(gp, cand, cn, &state_bytes));
    const size_t slot_off = (size_t)round_up64((int64_t)state_bytes, 256);
    if (!c->h_chain) ROBO_HIP_CHECK(hipHostMalloc((void**)&c->h_chain, ROBO_CHAIN_SLOTS * sizeof(unsigned), 0));
    unsigned* state = reinterpret_cast<unsigned*>(cand->d_chain);
    double* slots = reinterpret_cast<double*>(cand->d_chain + slot_off);
    const Tuning& tune = c->tune;
    const unsigned spin_limit = tune.trsm_chain_spin_limit >= 0 ? (unsigned)tune.trsm_chain_spin_limit : PROG_SPIN_LIMIT;
    const bool deep = tune.trsm_small_deep >= 0 ? tune.trsm_small_deep != 0 : wgs <= c->num_cu;
    // the acquisition screen's gather has zeroed exactly this block already (screen.hip): every other call keeps the memset
    if (cand->chain_cleared != state_bytes) ROBO_HIP_CHECK(hipMemsetAsync(state, 0, state_bytes, c->stream));
    cand->chain_cleared = 0;
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
