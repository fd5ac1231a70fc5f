// The 128 x 128 diagonal block of the blocked Cholesky (potrf.hip) as device functions: the block-packed LDS image, the
// 16-pivot block factorisation, the left-looking 128-pivot schedule with its publication to the panel followers.
// Shared by the factorisation's kernels (potrf.hip), the one-launch ensemble half-step (mcmc_block.hip) and the fragment
// packing of kept factors (fit_keep.hip: pi16).
#pragma once
#include "common.h"

namespace robo {

// ------------------------------------------------------------------------------------
// Diagonal block: 128x128, processed as 8x8 sub-blocks of 16x16 kept block-packed in LDS
// (lower blocks only: 36 blocks each for L and for W = L^-1).
// ------------------------------------------------------------------------------------
constexpr int SB = 16;                 // sub-block edge
constexpr int NSB = NB / SB;           // 8
constexpr int NBLK = NSB * (NSB + 1) / 2;   // 36
constexpr int BLK = SB * SB;           // 256 doubles

__device__ __forceinline__ int blk_off(int bi, int bj) { return (bi * (bi + 1) / 2 + bj) * BLK; }

// Element (r, c) of a 16x16 LDS block.  Rows are 16 doubles apart, so a plain row-major block puts
// the 16 rows of an MFMA A-fragment read (lane l -> row l & 15, column 4 kk + (l >> 4)) on only two
// 8-byte bank groups: an 8-way conflict on every fragment read (r01s: 1.4k cycles per 16x16x16
// product).  XOR-ing the column with (r & 14) spreads the 64 lanes of an A-fragment read, a
// B-fragment read and a C-layout access evenly over the 32 bank groups (2 lanes each = the minimum
// for a 512-byte wave access), at no cost in space -- the two images of the diagonal block already
// take 147 of the 160 KB.
__device__ __forceinline__ int bidx(int r, int c) { return r * SB + (c ^ (r & 14)); }

// LDS ops of one wave execute in order; this only stops the compiler from moving a
// cross-lane LDS read above the write it depends on (no instruction is emitted).
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// C-layout <-> LDS 16x16 block (row-major, ld 16)
__device__ __forceinline__ v4d blk_load_c(const double* b, int lane) {
    v4d c;
#pragma unroll
    for (int r = 0; r < 4; ++r) c[r] = b[bidx((lane >> 4) + 4 * r, lane & 15)];
    return c;
}
__device__ __forceinline__ void blk_store_c(double* b, int lane, v4d c) {
#pragma unroll
    for (int r = 0; r < 4; ++r) b[bidx((lane >> 4) + 4 * r, lane & 15)] = c[r];
}
// acc += sgn * A(16x16) * B^T(16x16)   ("NT": both blocks indexed [row][k])
template <bool NEG>
__device__ __forceinline__ v4d blk_mma_nt(const double* A, const double* B, int lane, v4d acc) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        double a = A[bidx(lane & 15, kk * 4 + (lane >> 4))];
        const double b = B[bidx(lane & 15, kk * 4 + (lane >> 4))];
        if (NEG) a = -a;
        acc = mfma_f64(a, b, acc);
    }
    return acc;
}
// acc += sgn * A(16x16) * B(16x16)     ("NN": B indexed [k][col])
template <bool NEG>
__device__ __forceinline__ v4d blk_mma_nn(const double* A, const double* B, int lane, v4d acc) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        double a = A[bidx(lane & 15, kk * 4 + (lane >> 4))];
        const double b = B[bidx(kk * 4 + (lane >> 4), lane & 15)];
        if (NEG) a = -a;
        acc = mfma_f64(a, b, acc);
    }
    return acc;
}

// fragments of a 16x16 LDS block for four consecutive MFMAs (k = 0..15): "row" form = element
// [lane & 15][4 kk + (lane >> 4)] (the A operand, and the B operand of an NT product), "col" form = element
// [4 kk + (lane >> 4)][lane & 15] (the B operand of an NN product)
struct Frag4 {
    double v[4];
};
__device__ __forceinline__ Frag4 frag_row(const double* A, int lane) {
    Frag4 f;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) f.v[kk] = A[bidx(lane & 15, kk * 4 + (lane >> 4))];
    return f;
}
__device__ __forceinline__ Frag4 frag_col(const double* B, int lane) {
    Frag4 f;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) f.v[kk] = B[bidx(kk * 4 + (lane >> 4), lane & 15)];
    return f;
}
template <bool NEG>
__device__ __forceinline__ v4d frag_mma(const Frag4& a, const Frag4& b, v4d acc) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) acc = mfma_f64(NEG ? -a.v[kk] : a.v[kk], b.v[kk], acc);
    return acc;
}

// broadcast lane `src`'s double to the whole wave through SGPRs (v_readlane_b32 x2; `src` is a
// compile-time constant after unrolling)
__device__ __forceinline__ double bcast_lane(double x, int src) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), src);
    return __hiloint2double(hi, lo);
}

// ---- 16x16 building blocks ------------------------------------------------------------
// Everything in the diagonal kernel is latency-bound on one pivot chain (128 sequential
// rsqrt -> scale -> update steps), so the blocks below are written for few instructions on that
// chain and for everything else to run on the other three waves meanwhile (measured with
// robo_selftest_diag_timeline: the first version spent 11.5k cycles per 16x16 potf2+inverse).

// 1 / sqrt(p) for a finite p > 0: v_rsq_f64 and one third-order correction r (1 + e/2 + 3 e^2/8), e = 1 - p r^2
// -- the sequence the compiler's rsqrt() expands to, minus its special-case selects (p = 0 / inf / NaN cannot
// reach this point: the pivot test above it replaces them, and an inf pivot only has to end in a flagged failure,
// which inf * 0 = NaN at the next pivot guarantees).
__device__ __forceinline__ double pivot_rsqrt(double p) {
    double r = __builtin_amdgcn_rsq(p);
    const double e = fma(-p * r, r, 1.0);
    return fma(r * e, fma(e, 0.375, 0.5), r);
}

// One wave: unblocked Cholesky of the 16x16 block Ld (lower part valid), in place, and its inverse W = L^-1 into Wd.
// g0 = global index of the block's first row; rows >= n_real have their pivot forced to 1 (augmented row and identity
// padding).  Returns the first failing global column + 1, or 0.
// The inverse costs no instruction of its own: half of the lanes run the SAME instruction stream on different data --
// instead of a row of the block they hold a column of W, started as a unit vector -- because the forward substitution
// L w = e_c is exactly "scale entry k by 1/L_kk, subtract column k of L times it from the entries below", i.e. the scale
// and update instructions of the factorisation with this lane's own multiplier.
// All four 16-lane groups are at work (r02w): a lane holds the entries of ONE COLUMN PARITY,
//     group 0: rows of L, even columns     group 2: rows of L, odd columns
//     group 1: columns of W, even rows     group 3: columns of W, odd rows
// i.e. 8 entries a[h] <-> second index j = 2 h + par, so the rank-1 update is at most 8 FMAs per pivot (with a whole row
// of 16 entries per lane on two lane groups the lone wave was bound by instruction ISSUE: ~34 instructions per pivot at
// ~10 cycles, a third of them the update), and the scaled column goes through LDS de-interleaved ([even rows | odd rows])
// so that a lane's operands are contiguous.
// The pivot chain does not pass through any lane's registers: the next diagonal entry with columns <= k-1 applied is
// broadcast as a uniform value d1 and  p_{k+1} = d1 - l_{k+1,k}^2  is one FMA on the broadcast l_{k+1,k} -- every
// entry of column k+1 (the diagonal one included) receives column k's contribution with the regular deferred update
// one iteration later, whose multiplier l_{row,k} a lane of the other parity reads back from the exchange buffer.
// colbuf: [4 groups][2 buffers][16], 1 KB.
// GUARD = false (every block that holds only training rows): the pivot is NOT tested on the chain.  A non-positive or NaN
// pivot makes v_rsq_f64 return NaN / inf, L_kk = p * rsqrt(p) comes out NaN, and so does everything after it -- the failing
// column is read off the diagonal once the block is done.  Four scalar/vector instructions and the select in front of the
// rsq less per pivot on an issue-bound wave; the scale needs no select either (a failed factorisation is flagged; its
// numbers are garbage either way).
template <bool GUARD>
__device__ __forceinline__ int potf2_16_split(double* Ld, double* Wd, double* colbuf, int lane, int g0, int n_real) {
    const int row = lane & 15, grp = lane >> 4, par = grp >> 1;
    const bool isW = (grp & 1) != 0;
    constexpr int H = SB / 2;
    double a[H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
        const int j = 2 * h + par;
        const double l = j <= row ? Ld[bidx(row, j)] : 0.0;
        a[h] = isW ? (j == row ? 1.0 : 0.0) : l;
    }
    const int pos = (row & 1) * H + (row >> 1);               // de-interleaved position of this lane's row
    double* cb_own = colbuf + grp * 2 * SB + pos;             // where this lane publishes its scaled entry
    const double* cb_mult = colbuf + (grp & 1) * 2 * SB + pos;   // + owner parity * 4 SB: this row's multiplier
    const double* cb_col = colbuf + par * H;                  // + owner parity * 4 SB: column values for own j's
    int fail = 0;
    double p = bcast_lane(a[0], 0);                           // L_00's pivot: group 0, lane 0
#pragma unroll
    for (int k = 0; k < SB; ++k) {
        const int pk = k & 1, hk = k >> 1;
        // (A) the exchange-buffer reads of the deferred update by column k-1 are ISSUED first and consumed last: the
        // column was published at the end of the previous iteration, so they are a full LDS write -> read round trip
        // away, and the compiler's own order put the pivot's fma + rsq chain behind the first s_waitcnt on them
        // (r03 ISA: ~290 cycles per pivot = LDS round trip + rsq chain + hand-over, one after the other).  With the
        // scheduling barriers the rsq chain of pivot k runs while the reads are in flight.
        double lprev = 0.0, cv[H];
        if (k > 0) {
            const int pq = (k - 1) & 1, buf = (k - 1) & 1;
            lprev = cb_mult[pq * 4 * SB + buf * SB];
            const double* c = cb_col + pq * 4 * SB + buf * SB;
#pragma unroll
            for (int h = hk; h < H; ++h) cv[h] = c[h];
        }
        __builtin_amdgcn_sched_barrier(0);
        // (B) the pivot
        if (GUARD) {
            if (g0 + k >= n_real) p = 1.0;
            if (!(p > 0.0)) {             // also catches NaN
                if (fail == 0) fail = g0 + k + 1;
                p = 1.0;
            }
        }
        const double ri = pivot_rsqrt(p);
        __builtin_amdgcn_sched_barrier(0);
        // (C) deferred update by column k-1 (owner parity pq) of every own column j >= k
        if (k > 0) {
#pragma unroll
            for (int h = hk; h < H; ++h) {
                // h = hk is column k for the lanes of parity pk; for the other parity it is column k+1 (k even) or the
                // finished column k-1 (k odd), which must not be touched
                const double m = (pk == 1 && h == hk) ? (par == 1 ? lprev : 0.0) : lprev;
                a[h] = fma(-m, cv[h], a[h]);
            }
        }
        // the next diagonal entry (columns <= k-1 applied), uniform: lane (row k+1, L group of parity (k+1) & 1)
        double d1 = 0.0;
        if (k + 1 < SB) d1 = bcast_lane(a[(k + 1) >> 1], (k + 1) + 32 * ((k + 1) & 1));
        double lik = a[hk] * ri;                              // meaningful in the lanes of parity pk
        if (GUARD && row == k && !isW) lik = p * ri;
        a[hk] = par == pk ? lik : a[hk];
        cb_own[(k & 1) * SB] = lik;                           // the other parity's copies are never read
        if (k + 1 < SB) {
            const double l1 = bcast_lane(lik, (k + 1) + 32 * pk);   // L[k+1][k]
            p = fma(-l1, l1, d1);
        }
        wave_lds_fence();
    }
    if (!GUARD) {
        // first column whose diagonal entry is not a positive finite number
        double diag = 0.0;
#pragma unroll
        for (int h = 0; h < H; ++h) diag = (row >> 1) == h ? a[h] : diag;
        const bool bad = !isW && par == (row & 1) && !(diag > 0.0 && diag < 1.0e300);
        const unsigned long long m = __ballot(bad);
        if (m != 0ull) fail = g0 + ((__ffsll((long long)m) - 1) & 15) + 1;
    }
#pragma unroll
    for (int h = 0; h < H; ++h) {
        const int j = 2 * h + par;
        if (isW) Wd[bidx(j, row)] = a[h];                     // W[j][c], zero above the diagonal
        else Ld[bidx(row, j)] = j <= row ? a[h] : 0.0;
    }
    return fail;
}

// (Two other forms were built and measured slower -- a whole row per lane on two lane groups, and rank-1 updates on the
// matrix pipe in LDL^T form, 5.8-6.0k cycles per 16 pivots against 3.8-4.3k here: NOTES.md r02w, r03t.)

// the pivot guard for rows >= n_real only exists in the block(s) that hold the augmented row / padding
__device__ __forceinline__ int potf2_16(double* Ld, double* Wd, double* colbuf, int lane, int g0, int n_real) {
    if (g0 + SB <= n_real) return potf2_16_split<false>(Ld, Wd, colbuf, lane, g0, n_real);
    return potf2_16_split<true>(Ld, Wd, colbuf, lane, g0, n_real);
}

constexpr int TLD = SB + 2;   // padded leading dimension of the per-wave transposition scratch

// ---- the 128x128 diagonal block, block-packed in LDS -------------------------------------
// sL: 36 lower 16x16 blocks of A -> L in place; sW: 36 blocks of W = L^-1; sT: per-wave 16 x TLD
// scratch; sRd: task counters of the helper waves (8 ints); sCol: 4 x 2 x 16 column exchange buffers (wave 0).
//
// LEFT-LOOKING schedule (r02): wave 0 is the pivot wave and does nothing but the chain
//      potf2(s) -> L_{s+1,s} = A~_{s+1,s} W_ss^T -> A~_{s+1,s+1} -= L_{s+1,s} L_{s+1,s}^T -> potf2(s+1)
// i.e. two 16x16x16 MFMA products between consecutive 16-pivot chains.  Every other product runs on
// waves 1-3 in the shadow of a potf2:  a block A_ij is touched exactly twice -- once to receive ALL its
// updates  A~_ij = A_ij - sum_{c<j} L_ic L_jc^T  (accumulated in registers, one LDS round trip), once for
// its solve with W_jj.  The right-looking form of r01 re-read and re-wrote every trailing 16x16 block at
// every step (27, 20, 14 ... blocks on three waves: the early steps took 11-13k cycles against the pivot
// wave's 6.4k) and put a four-wave sub-panel phase plus a barrier on the chain.
// Interval s (two barriers, Ba at its start right after potf2(s), Bb in the middle):
//   wave 0     : C1  L_{s+1,s};  C2  pivot block (s+1,s+1) finished;  [Bb]  potf2(s+1)
//   waves 1-3  : solves L_{i,s}, i >= s+2   [Bb]   block column s+1 and pivot block (s+2,s+2) receive all
//                their updates (columns 0..s); the inverse advances by block row s, column by column (see the
//                task list in the loop).  One product per block of row 7 of W is left after the last pivot.
// ---- publication for the panel followers (potrf_step_follow_kernel) ---------------------------------------------------------
// With pub != nullptr the diagonal workgroup hands block column s of L_kk and W_ss to the OTHER workgroups of its launch as
// soon as they are final (after barrier Bb(s)), straight into their final places in K and in the inverse block -- so the
// write-back at the end goes away -- with write-through stores by the three helper waves, issued at the START of their
// half-interval (the pivot wave stores nothing: its chain is untouched).  The progress word COUNTS publications: every
// helper wave adds 1 once ITS stores of column s have left the CU -- no barrier between the three -- so column c is in memory
// when the word reads >= 3 (c + 1).  When: in the first intervals the helpers are the longer side of the interval (their
// update tasks, r05z_diag_timeline), so they drain and count AFTER their tasks, when the stores have long completed; from
// interval `early` on (potrf_pub_early, default 5: one or no task per wave) they have time to spare and count at once -- the followers then work on column s while the pivot
// wave runs potf2(s+1), and only the last column (16 x 16: W_77) is left when the diagonal block ends.  After the last pivot
// all four waves publish what the loop did not (column nsb - 1 and the identity padding) and add 1 each:
// the word ends at 3 (nsb - 1) + 4 = diag_prog_done(nsb).  Same arithmetic, same bits.
__host__ __device__ constexpr unsigned diag_prog_need(int c, int nsb) {      // value of the progress word from which column c is readable
    return c < nsb - 1 ? 3u * (unsigned)(c + 1) : 3u * (unsigned)(nsb - 1) + 4u;
}
__host__ __device__ constexpr int diag_nsb(int n_real, int kbase) {          // 16-row blocks of a diagonal block that are factored
    const int v = (n_real + 1 - kbase + SB - 1) / SB;
    return v < 1 ? 1 : (v > NSB ? NSB : v);
}
struct DiagPub {
    double* Kd;        // tile (k, k) in K (row-major, leading dimension ld)
    int ld;
    double* Wg;        // the 128 x 128 inverse block of panel k (its eight diagonal sub-blocks are written)
    unsigned* prog;    // progress word of panel k
    int early;         // first interval whose helper waves count right after publishing (see below)
};
// one wave: 16 x 16 LDS block (bidx layout) -> 16 rows of a row-major global matrix, write-through
__device__ __forceinline__ void blk_publish(const double* b, double* dst, int ld, int lane) {
    const int r = lane >> 2, c0 = (lane & 3) * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) st_agent(dst + (size_t)r * ld + c0 + q, b[bidx(r, c0 + q)]);
}
// block column c of L (rows c .. 7) and W_cc, blocks dealt round-robin to `nw` waves (this wave: `w`)
// (Wc: the LDS block that holds W_cc, or nullptr: the identity -- a padding block of the rolling layout, which keeps no image of W)
__device__ __forceinline__ void diag_publish_column(const double* sL, const double* Wc, const DiagPub& pub, int c, int w,
                                                    int nw, int lane) {
    int t = 0;
    for (int bi = c; bi < NSB; ++bi, ++t)
        if (t % nw == w) blk_publish(sL + blk_off(bi, c), pub.Kd + (size_t)(bi * SB) * pub.ld + c * SB, pub.ld, lane);
    if (t % nw == w) {
        double* dst = pub.Wg + (size_t)(c * SB) * NB + c * SB;
        if (Wc) {
            blk_publish(Wc, dst, NB, lane);
        } else {
            const int r = lane >> 2, c0 = (lane & 3) * 4;
#pragma unroll
            for (int q = 0; q < 4; ++q) st_agent(dst + (size_t)r * NB + c0 + q, r == c0 + q ? 1.0 : 0.0);
        }
    }
}

// ROLL (publishing callers only): sW is TWO 16 x 16 slots instead of a 36-block image -- W_ss lives in slot s & 1 from
// potf2(s) until it has been published (interval s), potf2(s + 2) may overwrite it a barrier later; the whole LDS image of a
// diagonal workgroup is then 80 KB (L image + 2 slots + exchange buffers): TWO workgroups per CU (r05g's layout, which had
// nowhere to put the W_ss; the publication gives them a place at once).
template <bool ROLL = false>
__device__ __forceinline__ void diag128_factor_invert(double* sL, double* sW, double* sT, double* sRd, double* sCol,
                                                      int kbase, int n_real, int* fail, long long* dbg,
                                                      const DiagPub* pub = nullptr) {
    auto wslot = [sW](int s_) { return ROLL ? sW + (s_ & 1) * BLK : sW + blk_off(s_, s_); };
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int* ctr = reinterpret_cast<int*>(sRd);     // one task counter per interval
    if (tid >= 64 && tid < 64 + NSB) ctr[tid - 64] = 0;
    // 16-row blocks that hold training rows or the augmented row; the ones behind them are identity padding (their
    // factor and inverse are the identity and nothing couples them to the rest), so the chain stops there: at the
    // N < 128 of a Bayesian-optimisation run the single diagonal block is mostly padding (N = 30: 2 of 8 blocks).
    const int nsb = diag_nsb(n_real, kbase);
    if (!ROLL)
        for (int bi = nsb; bi < NSB; ++bi) sW[blk_off(bi, bi) + bidx(tid >> 4, tid & 15)] = (tid >> 4) == (tid & 15) ? 1.0 : 0.0;
    // this lane's offsets inside a 16x16 block: fragment form [lane & 15][4 kk + (lane >> 4)], accumulator form
    // [(lane >> 4) + 4 r][lane & 15]
    int fo[4], co[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        fo[q] = bidx(lane & 15, q * 4 + (lane >> 4));
        co[q] = bidx((lane >> 4) + 4 * q, lane & 15);
    }
    if (wave == 0) {
        const int f = potf2_16(sL + blk_off(0, 0), wslot(0), sCol, lane, kbase, n_real);
        if (f != 0 && lane == 0 && *fail == 0) *fail = f;
    }
    __syncthreads();                                              // Ba(0)
    if (dbg && tid == 0) dbg[2] = clock64();
    for (int s = 0; s + 1 < nsb; ++s) {
        if (wave == 0) {
            // C1: the TRANSPOSE Q = L_{s+1,s}^T = W_ss A~_{s+1,s}^T.  In the MFMA accumulator layout register r
            // of lane l holds Q[(l >> 4) + 4 r][l & 15], which is at once the A fragment of columns 4r..4r+3 of Q^T
            // and the B fragment of rows 4r..4r+3 of Q:
            // C2: the pivot block's last update  T -= L L^T = Q^T Q  is four MFMAs straight from those registers,
            // with no trip through LDS between the two products of the chain.
            double* P = sL + blk_off(s + 1, s);
            double* C = sL + blk_off(s + 1, s + 1);
            v4d t = blk_load_c(C, lane);
            v4d q = {0.0, 0.0, 0.0, 0.0};
            q = blk_mma_nt<false>(wslot(s), P, lane, q);
#pragma unroll
            for (int r = 0; r < 4; ++r) t = mfma_f64(-q[r], q[r], t);
            blk_store_c(C, lane, t);
            wave_lds_fence();   // (also orders the fragment reads of P before its overwrite)
#pragma unroll
            for (int r = 0; r < 4; ++r) P[bidx(lane & 15, (lane >> 4) + 4 * r)] = q[r];   // L = Q^T for the helpers
            wave_lds_fence();
            if (dbg && tid == 0) dbg[24 + 4 * s] = clock64();     // C1 + C2 done (pivot wave)
        } else {
            // solves of block column s below the pivot wave's own block
            for (int bi = s + 2 + (wave - 1); bi < nsb; bi += 3) {
                double* A = sL + blk_off(bi, s);
                v4d acc = {0.0, 0.0, 0.0, 0.0};
                acc = blk_mma_nt<false>(A, wslot(s), lane, acc);
                wave_lds_fence();
                blk_store_c(A, lane, acc);
            }
        }
        __syncthreads();                                          // Bb(s): block column s of L is final
        if (dbg && tid == 0 && s == 0) dbg[3] = clock64();
        if (dbg && tid == 0) dbg[24 + 4 * s + 1] = clock64();     // through Bb(s)
        if (pub && wave != 0) {
            diag_publish_column(sL, wslot(s), *pub, s, wave - 1, 3, lane);
            if (s >= pub->early) {
                drain_vmem();
                if (lane == 0) add_agent_u32(pub->prog, 1u);
            }
        }
        if (wave == 0) {
            const int f = potf2_16(sL + blk_off(s + 1, s + 1), wslot(s + 1), sCol, lane,
                                   kbase + (s + 1) * SB, n_real);
            if (f != 0 && lane == 0 && *fail == 0) *fail = f;
            if (dbg && tid == 0) dbg[24 + 4 * s + 2] = clock64() + (long long)(f == 12345678);   // potf2(s+1) done
        } else {
            // Work of the interval, handed out dynamically (an LDS counter per interval; a task is wave-sized):
            // one block of column s+1 (or the next pivot block) receives columns 0..s in one pass.
            // t = 0: (s+2, s+1) and t = 1: (s+2, s+2) are what the pivot wave needs first at the next
            // interval; t >= 2: (s+1+t, s+1).
            // The off-diagonal blocks of the inverse W = L^-1 are NOT formed here (r02f): advanced alongside the
            // factorisation they cost 112 more 16x16x16 products on these three waves and made the pivot wave
            // wait (84.7k cycles per diagonal block against 68.2k without them).  The panel solve needs only the
            // eight W_ss that fall out of potf2 (potrf_panel_kernel substitutes block column by block column);
            // the full inverses, which the posterior's TRSM and the likelihood gradient use, are produced for
            // all diagonal blocks at once by potrf_inverse_kernel after the factorisation.
            // Static hand-out (task t to wave 1 + t % 3), lane offsets computed once per kernel.  (Dynamic hand-out
            // through an LDS counter, pairing blocks that share an operand, and software-pipelined fragment loads
            // were all measured within noise of this: intervals 1-3 take 6.0-7.2k cycles against 4.5k for the pivot
            // wave alone, whatever the bookkeeping -- the pivot wave's own LDS exchange slows down while the helpers'
            // fragment reads share the LDS pipe.)
            const int ntask = s + 2 < nsb ? nsb - 1 - s : 0;
            for (int t = wave - 1; t < ntask; t += 3) {
                const int bi = t <= 1 ? s + 2 : s + 1 + t;
                const int bj = t == 1 ? s + 2 : s + 1;
                double* C = sL + blk_off(bi, bj);
                const double* Ai = sL + blk_off(bi, 0);
                const double* Bj = sL + blk_off(bj, 0);
                v4d acc;
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] = C[co[r]];
                for (int c = 0; c <= s; ++c) {
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) acc = mfma_f64(-Ai[c * BLK + fo[kk]], Bj[c * BLK + fo[kk]], acc);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) C[co[r]] = acc[r];
            }
        }
        if (pub && wave != 0 && s < pub->early) {
            drain_vmem();                                         // this wave's share of column s has left the CU
            if (lane == 0) add_agent_u32(pub->prog, 1u);
        }
        __syncthreads();                                          // Ba(s+1)
        if (dbg && tid == 0) dbg[4 + s] = clock64();
    }
    if (pub) {
        // what the loop did not hand over: the last factored block column (nsb - 1) and the identity padding behind it
        for (int c = nsb - 1; c < NSB; ++c)
            diag_publish_column(sL, (ROLL && c >= nsb) ? nullptr : wslot(c), *pub, c, wave, 4, lane);
        drain_vmem();
        if (lane == 0) add_agent_u32(pub->prog, 1u);
    }
    if (dbg && tid == 0) dbg[11] = clock64();
}

constexpr int DIAG_SMEM_DOUBLES = 2 * NBLK * BLK + 4 * SB * TLD + NB + 8 * SB;   // 150 KB

struct DiagSmem {
    double *sL, *sW, *sT, *sRd, *sCol;
};
__device__ __forceinline__ DiagSmem diag_carve(double* base) {
    DiagSmem m;
    m.sL = base;
    m.sW = m.sL + NBLK * BLK;
    m.sT = m.sW + NBLK * BLK;
    m.sRd = m.sT + 4 * SB * TLD;
    m.sCol = m.sRd + NB;
    return m;
}

// L into K (lower sub-blocks); the eight W_ss = L_ss^-1 into the diagonal sub-blocks of the 128x128 row-major
// inverse block (its off-diagonal sub-blocks are filled in by potrf_inverse_kernel; the strictly upper ones were
// zeroed when the buffer was allocated and are never written)
__device__ __forceinline__ void diag_writeback(const DiagSmem& m, double* __restrict__ Kd, int ld,
                                               double* __restrict__ Wg) {
    const int tid = threadIdx.x;
    for (int bi = 0; bi < NSB; ++bi) {
        for (int bj = 0; bj <= bi; ++bj) {
            const int r = bi * SB + (tid >> 4), c = bj * SB + (tid & 15);
            Kd[(size_t)r * ld + c] = m.sL[blk_off(bi, bj) + bidx(tid >> 4, tid & 15)];
        }
        const int r = bi * SB + (tid >> 4), c = bi * SB + (tid & 15);
        Wg[r * NB + c] = m.sW[blk_off(bi, bi) + bidx(tid >> 4, tid & 15)];
    }
}

// the 36 lower sub-blocks of the row-major tile Kd into the block-packed image sL (all 256 threads, one element per block)
__device__ __forceinline__ void diag_load_lower(double* sL, const double* Kd, int ld) {
    const int tid = threadIdx.x;
    for (int bi = 0; bi < NSB; ++bi)
        for (int bj = 0; bj <= bi; ++bj)
            sL[blk_off(bi, bj) + bidx(tid >> 4, tid & 15)] = Kd[(size_t)(bi * SB + (tid >> 4)) * ld + bj * SB + (tid & 15)];
}

// Within every 16-block the panel kernel indexes panel columns through the 4x4 index transpose pi(a) = (a >> 2) | ((a & 3) << 2)
// (an involution): register r of lane (i = l & 15, g = l >> 4) of an accumulator-layout Y_s is then X[strip row i][16 s + 4 g + r],
// i.e. FOUR CONSECUTIVE doubles of the strip's row -- the strip is loaded and stored with 16-byte accesses (r02o: the
// 8-byte column-strided form cost 11.2k cycles of loads and 7k of stores around a 11.8k-cycle chain).  The LDS images of
// L_sc and W_ss are permuted the same way in rows and columns when they are staged, which costs nothing.
__device__ __forceinline__ constexpr int pi16(int a) { return (a >> 2) | ((a & 3) << 2); }
__device__ __forceinline__ constexpr int tri_row(int b) {      // block index -> (bi, bj) of blk_off, compile time
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= b) ++i;
    return i;
}

}  // namespace robo
