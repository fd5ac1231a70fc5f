// DIRECT over a closed-form acquisition, resident on the device: the kernels (robo_acq_direct, robo_acq_direct_marginal; the
// rule is stated in include/robo_hip.h, the driver is api_direct.hip).
//
// The reference's Direct maximiser (robo/maximizers/direct.py) drives the DIRECT package from the host, one 1 x D acquisition
// call per function value.  Here one iteration is four launches around the posterior of its B points:
//
//   dir_classmin_kernel  grid-wide segmented reduction over the rectangle store: every workgroup takes DIR_CHUNK rectangles
//                        and keeps the (value, index) minimum of every size class in LDS -- the value as an order-preserving
//                        64-bit key under ds_min_u64, then the lowest index among the rectangles that hold that key -- and
//                        writes its table out.  Minima of (key, index) pairs are exact, so the merged table does not depend
//                        on how the store was cut into workgroups
//   dir_select_kernel    ONE workgroup: merges the tables in workgroup order into LDS (which also yields fmin and the best
//                        rectangle), runs the all-pairs test of potential optimality with one lane per class, prefix-sums
//                        (taken, slots) with a wave scan, defers what passes B rows, and writes the points c +- delta e_i,
//                        a wave per rectangle, scaled by every model's metrics into that model's candidate handle
//   (per model)          the posterior of the B rows: predict_scaled, as robo_acq_eval runs it for such a batch
//   dir_divide_kernel    a wave per taken rectangle: values from the resident moments (mean over the models in order),
//                        w_i = min(f+, f-), ranking by counting, the children appended at n_before + slot, the parent's
//                        levels and class moved on
//   dir_result_kernel    the best rectangle from a last merge, the counters and flags, the trace's copy of the store
//
// dir_init_kernel and dir_divide_kernel(t = 0) make rectangle 0 from the centre.  Everything a later kernel decides on is in
// DirState::hdr; a stop is a word there that every kernel of this file reads first.
#include "kern_math.h"

namespace robo {

constexpr double DIR_DBL_MAX = 1.79769313486231570e308;
constexpr unsigned long long DIR_KEY_EMPTY = ~0ull, DIR_SIGN = 0x8000000000000000ull;
constexpr int DIR_IDX_EMPTY = 0x7FFFFFFF;
constexpr int DIR_PACK = 20;        // the select kernel scans (taken << DIR_PACK | slots): slots < 2^20, taken < 2^11

// f is never NaN and never -0: key order is value order and equal keys are equal values
__device__ __forceinline__ unsigned long long dir_key(double f) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(f);
    return (b & DIR_SIGN) ? ~b : b | DIR_SIGN;
}
__device__ __forceinline__ double dir_unkey(unsigned long long k) {
    return __longlong_as_double((long long)((k & DIR_SIGN) ? k & ~DIR_SIGN : ~k));
}
__device__ __forceinline__ double dir_f(double a) {
    if (a != a) return DIR_DBL_MAX;
    if (a == 0.0) return 0.0;
    const double f = -a;
    return f > DIR_DBL_MAX ? DIR_DBL_MAX : (f < -DIR_DBL_MAX ? -DIR_DBL_MAX : f);
}

// the acquisition value of row `at` of the models' handles: the mean over the models in order, guards as acq_kernel's
__device__ __forceinline__ double dir_value(const DirState& st, size_t at) {
    double facc = 0.0;
    unsigned f = 0;
    for (int s = 0; s < st.S; ++s) {
        const CmaModel md = st.model[s];
        const double mean = md.mean[at], v = md.var[at];
        double lp;
        if (st.kind == ROBO_ACQ_EI) {
            lp = acq_ei(mean, v, md.eta, st.par);
            if (lp < 0.0 && lp > -2.2250738585072014e-308) lp = 0.0;
            if (lp < 0.0) f |= ROBO_FLAG_NEGATIVE_EI;
        } else if (st.kind == ROBO_ACQ_LOG_EI) {
            lp = acq_log_ei(mean, v, md.eta, st.par);
        } else if (st.kind == ROBO_ACQ_PI) {
            lp = acq_pi(mean, v, md.eta, st.par);
        } else {
            lp = acq_lcb(mean, v, st.par);
        }
        if (sqrt(v) == 0.0) f |= ROBO_FLAG_ZERO_SIGMA;
        facc = s > 0 ? facc + lp : lp;
    }
    const double val = rn_div(facc, (double)st.S);
    if (val != val) f |= ROBO_FLAG_NAN;
    if (f != 0) atomicOr(st.flags, f);
    return val;
}

// the (key, index) minimum over the first `parts` tables of class s, in workgroup order
__device__ __forceinline__ void dir_merge(const DirState& st, int parts, int s, unsigned long long& key, int& idx) {
    key = DIR_KEY_EMPTY;
    idx = DIR_IDX_EMPTY;
    for (int b = 0; b < parts; ++b) {
        const unsigned long long k = st.part_key[(size_t)b * st.n_cls + s];
        const int i = st.part_idx[(size_t)b * st.n_cls + s];
        if (k < key || (k == key && i < idx)) {
            key = k;
            idx = i;
        }
    }
}

// the lowest (key, index) pair of the workgroup's lanes -> every lane; sK, sI: WG entries
__device__ __forceinline__ void dir_block_min(unsigned long long* sK, int* sI, unsigned long long& key, int& idx) {
    const int tid = threadIdx.x;
    sK[tid] = key;
    sI[tid] = idx;
    __syncthreads();
    for (int o = WG / 2; o > 0; o >>= 1) {
        if (tid < o && (sK[tid + o] < sK[tid] || (sK[tid + o] == sK[tid] && sI[tid + o] < sI[tid]))) {
            sK[tid] = sK[tid + o];
            sI[tid] = sI[tid + o];
        }
        __syncthreads();
    }
    key = sK[0];
    idx = sI[0];
    __syncthreads();
}

__device__ __forceinline__ void dir_trace_head(double* row, double ran, int npo, int nslots, int n_before, int evals, double fmin,
                                               int best, unsigned flags) {
    row[0] = ran;
    row[1] = (double)npo;
    row[2] = (double)nslots;
    row[3] = (double)n_before;
    row[4] = (double)evals;
    row[5] = fmin;
    row[6] = (double)best;
    row[7] = (double)flags;
}

// iteration 0: the centre into every row of the batch and of every model's handle
__global__ __launch_bounds__(WG) void dir_init_kernel(DirState st) {
    const int tid = threadIdx.x, D = st.D, B = st.B;
    for (int e = tid; e < B * D; e += WG) st.x[e] = 0.5;
    for (int s = 0; s < st.S; ++s) {
        const CmaModel md = st.model[s];
        for (long long e = tid; e < st.m_pad * D; e += WG) md.Xcs[e] = 0.5 * md.ism[e % D];
    }
    if (tid == 0) {
        st.hdr[DIR_N_RECT] = 1;
        st.hdr[DIR_EVALS] = 1;
        st.hdr[DIR_ITERS] = 0;
        st.hdr[DIR_STOP] = 0;
        st.hdr[DIR_N_BEFORE] = 0;
        st.hdr[DIR_N_SLOTS] = 1;
        st.hdr[DIR_N_PO] = 0;
        st.hdr[DIR_BEST] = -1;
        st.fbest[0] = 0.0;
        *st.flags = 0u;
    }
    if (!st.trace) return;
    double* row = st.trace;
    if (tid == 0) dir_trace_head(row, 1.0, 0, 1, 0, 1, 0.0, -1, 0u);
    for (int e = tid; e < B / 2; e += WG) row[8 + e] = -1.0;
    for (int e = tid; e < B * D; e += WG) row[8 + B / 2 + e] = 0.5;
    for (int e = tid; e < B; e += WG) row[8 + B / 2 + (size_t)B * D + e] = 0.0;
}

__global__ __launch_bounds__(WG) void dir_classmin_kernel(DirState st, int force) {
    __shared__ unsigned long long sKey[DIR_NCLS_MAX];
    __shared__ int sIdx[DIR_NCLS_MAX];
    if (!force && st.hdr[DIR_STOP] != 0) return;
    const int tid = threadIdx.x, n = st.hdr[DIR_N_RECT], r0 = blockIdx.x * DIR_CHUNK;
    if (r0 >= n) return;
    const int r1 = n < r0 + DIR_CHUNK ? n : r0 + DIR_CHUNK;
    for (int s = tid; s < st.n_cls; s += WG) {
        sKey[s] = DIR_KEY_EMPTY;
        sIdx[s] = DIR_IDX_EMPTY;
    }
    __syncthreads();
    for (int r = r0 + tid; r < r1; r += WG) atomicMin(&sKey[st.cls[r]], dir_key(st.f[r]));
    __syncthreads();
    for (int r = r0 + tid; r < r1; r += WG) {
        const int s = st.cls[r];
        if (dir_key(st.f[r]) == sKey[s]) atomicMin(&sIdx[s], r);
    }
    __syncthreads();
    for (int s = tid; s < st.n_cls; s += WG) {
        st.part_key[(size_t)blockIdx.x * st.n_cls + s] = sKey[s];
        st.part_idx[(size_t)blockIdx.x * st.n_cls + s] = sIdx[s];
    }
}

__global__ __launch_bounds__(WG) void dir_select_kernel(DirState st, int t) {
    __shared__ double sF[DIR_NCLS_MAX];
    __shared__ int sR[DIR_NCLS_MAX], sScan[DIR_NCLS_MAX];
    __shared__ unsigned long long sRedK[WG];
    __shared__ int sRedI[WG], sWave[WG / 64], sDim[WG / 64][DIR_MAX_DIM];
    __shared__ int s_npo, s_nslots, s_deferred;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, D = st.D, B = st.B, ncls = st.n_cls;
    double* row = st.trace ? st.trace + (size_t)t * dir_trace_row(D, B) : nullptr;
    const int n = st.hdr[DIR_N_RECT], evals = st.hdr[DIR_EVALS];
    int stop = st.hdr[DIR_STOP];
    if (stop == 0) {
        if (evals >= st.max_evals) stop = (int)ROBO_DIRECT_STOP_BUDGET;
        else if (n + B > st.cap) stop = (int)ROBO_DIRECT_STOP_CAPACITY;
    }
    if (tid == 0) {
        s_npo = 0;
        s_nslots = 0;
        s_deferred = 0;
    }
    double f_min = 0.0;
    int best = -1;
    if (stop == 0) {
        // ---- merge: class minima into LDS; f_min and the best over ALL classes
        const int parts = (n + DIR_CHUNK - 1) / DIR_CHUNK;
        unsigned long long bk = DIR_KEY_EMPTY;
        int bi = DIR_IDX_EMPTY;
        for (int s = tid; s < ncls; s += WG) {
            unsigned long long k;
            int i;
            dir_merge(st, parts, s, k, i);
            sF[s] = dir_unkey(k);
            sR[s] = i == DIR_IDX_EMPTY ? -1 : i;
            if (k < bk || (k == bk && i < bi)) {
                bk = k;
                bi = i;
            }
        }
        dir_block_min(sRedK, sRedI, bk, bi);
        f_min = dir_unkey(bk);
        best = bi;
        // ---- all pairs, one lane per class with k < LMAX (the last class is the indivisible one)
        const double afmin = fabs(f_min), inf = __builtin_huge_val();
        for (int j = tid; j < ncls; j += WG) {
            int v = 0;
            if (j < ncls - 1 && sR[j] >= 0) {
                const double Fj = sF[j], dj = st.dsz[j];
                double khi = inf, klo = 0.0;
                for (int i = 0; i < ncls - 1; ++i) {
                    if (i == j || sR[i] < 0) continue;
                    if (i < j) khi = fmin(khi, rn_div(rn_sub(sF[i], Fj), rn_sub(st.dsz[i], dj)));
                    else klo = fmax(klo, rn_div(rn_sub(Fj, sF[i]), rn_sub(dj, st.dsz[i])));
                }
                bool po = khi > 0.0 && klo <= khi;
                if (po && khi != inf) {
                    if (f_min != 0.0) po = st.eps <= rn_add(rn_div(rn_sub(f_min, Fj), afmin), rn_mul(rn_div(dj, afmin), khi));
                    else po = Fj <= rn_mul(dj, khi);
                }
                if (po) v = (1 << DIR_PACK) | (2 * (D - j % D));
            }
            sScan[j] = v;
        }
        __syncthreads();
        // ---- exclusive prefix of (taken, slots) in class order: a serial run per lane, a wave scan, the waves' totals
        const int ipl = (ncls + WG - 1) / WG, a0 = tid * ipl < ncls ? tid * ipl : ncls, a1 = a0 + ipl < ncls ? a0 + ipl : ncls;
        int sum = 0;
        for (int s = a0; s < a1; ++s) sum += sScan[s];
        int inc = sum;
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(inc, o);
            if (lane >= o) inc += up;
        }
        if (lane == 63) sWave[wave] = inc;
        __syncthreads();
        int base = inc - sum;
        for (int w = 0; w < wave; ++w) base += sWave[w];
        for (int s = a0; s < a1; ++s) {
            const int v = sScan[s];
            if (v == 0) continue;
            const int q = base >> DIR_PACK, off = base & ((1 << DIR_PACK) - 1), cnt = v & ((1 << DIR_PACK) - 1);
            if (off + cnt <= B) {            // (monotone in class order: the first that does not fit defers all later ones)
                st.po_rect[q] = sR[s];
                st.po_off[q] = off;
                atomicMax(&s_npo, q + 1);
                atomicMax(&s_nslots, off + cnt);
            } else {
                s_deferred = 1;
            }
            base += v;
        }
        __syncthreads();
        if (s_npo == 0) stop = (int)ROBO_DIRECT_STOP_NOTHING;
    }
    const int npo = stop == 0 ? s_npo : 0, nslots = stop == 0 ? s_nslots : 0;
    if (tid == 0) {
        st.hdr[DIR_STOP] = stop;
        st.hdr[DIR_N_BEFORE] = n;
        st.hdr[DIR_N_SLOTS] = nslots;
        st.hdr[DIR_N_PO] = npo;
        if (stop == 0) {
            st.hdr[DIR_N_RECT] = n + nslots;
            st.hdr[DIR_EVALS] = evals + nslots;
            st.hdr[DIR_ITERS] += 1;
            st.hdr[DIR_BEST] = best;
            st.fbest[0] = f_min;
            if (s_deferred) atomicOr(st.flags, ROBO_DIRECT_DEFERRED);
        }
    }
    if (row) {
        if (tid == 0)
            dir_trace_head(row, stop == 0 ? 1.0 : 0.0, npo, nslots, n, evals + nslots, stop == 0 ? f_min : st.fbest[0],
                           stop == 0 ? best : st.hdr[DIR_BEST], (unsigned)stop | *st.flags | (s_deferred ? ROBO_DIRECT_DEFERRED : 0u));
        for (int e = tid; e < B / 2; e += WG) row[8 + e] = e < npo ? (double)st.po_rect[e] : -1.0;
        for (int e = tid; e < B; e += WG) row[8 + B / 2 + (size_t)B * D + e] = 0.0;
        if (stop != 0)
            for (int e = tid; e < B * D; e += WG) row[8 + B / 2 + e] = st.x[e];
    }
    if (stop != 0) return;
    // ---- emit: a wave per taken rectangle; lane d stages the dimensions of I in order, then the wave writes the rows
    double* tx = row ? row + 8 + B / 2 : nullptr;
    for (int q0 = 0; q0 < npo; q0 += WG / 64) {
        const int q = q0 + wave;
        int r = 0, off = 0, k = 0, nI = 0;
        if (q < npo) {
            r = st.po_rect[q];
            off = st.po_off[q];
            const int s = st.cls[r];
            k = s / D;
            nI = D - s % D;
            if (lane < D && st.lev[(size_t)r * D + lane] == k) {
                int pos = 0;
                for (int i = 0; i < lane; ++i) pos += st.lev[(size_t)r * D + i] == k ? 1 : 0;
                sDim[wave][pos] = lane;
            }
        }
        __syncthreads();
        const double dl = st.delta[k + 1];
        for (int e = lane; e < 2 * nI * D; e += 64) {
            const int slot = e / D, d = e - slot * D;
            const double cv = st.c[(size_t)r * D + d];
            const double xv = d != sDim[wave][slot >> 1] ? cv : ((slot & 1) ? cv - dl : cv + dl);
            const size_t at = (size_t)(off + slot) * D + d;
            st.x[at] = xv;
            for (int s = 0; s < st.S; ++s) st.model[s].Xcs[at] = xv * st.model[s].ism[d];
            if (tx) tx[at] = xv;
        }
        __syncthreads();
    }
    // rows beyond the used slots replicate row 0, as scale_inputs_kernel's pad rows do
    const long long first = (long long)nslots * D;
    for (long long e = first + tid; e < (long long)B * D; e += WG) {
        st.x[e] = st.x[e % D];
        if (tx) tx[e] = st.x[e % D];
    }
    for (int s = 0; s < st.S; ++s) {
        double* X = st.model[s].Xcs;
        for (long long e = first + tid; e < st.m_pad * D; e += WG) X[e] = X[e % D];
    }
}

// one wave per taken rectangle (t = 0: workgroup 0 makes rectangle 0 from the centre's value)
__global__ __launch_bounds__(64) void dir_divide_kernel(DirState st, int t) {
    __shared__ int sPos[DIR_MAX_DIM], sRank[DIR_MAX_DIM];
    __shared__ double sW[DIR_MAX_DIM];
    __shared__ int sLev[DIR_MAX_DIM];
    const int q = blockIdx.x, lane = threadIdx.x, D = st.D, B = st.B;
    double* tval = st.trace ? st.trace + (size_t)t * dir_trace_row(D, B) + 8 + B / 2 + (size_t)B * D : nullptr;
    if (t == 0) {
        if (q != 0) return;
        if (lane < D) {
            st.c[lane] = 0.5;
            st.lev[lane] = 0;
        }
        if (lane == 0) {
            const double a = dir_value(st, 0);
            st.f[0] = dir_f(a);
            st.cls[0] = 0;
            if (tval) tval[0] = a;
        }
        return;
    }
    if (q >= st.hdr[DIR_N_PO]) return;
    const int r = st.po_rect[q], off = st.po_off[q], n0 = st.hdr[DIR_N_BEFORE], s = st.cls[r], k = s / D, nI = D - s % D;
    if (lane < D) sLev[lane] = st.lev[(size_t)r * D + lane];
    __syncthreads();
    if (lane < D) {
        int pos = 0;
        for (int i = 0; i < lane; ++i) pos += sLev[i] == k ? 1 : 0;
        sPos[lane] = sLev[lane] == k ? pos : -1;
    }
    if (lane < nI) {
        const double ap = dir_value(st, (size_t)off + 2 * lane), am = dir_value(st, (size_t)off + 2 * lane + 1);
        const double fp = dir_f(ap), fm = dir_f(am);
        st.f[n0 + off + 2 * lane] = fp;
        st.f[n0 + off + 2 * lane + 1] = fm;
        sW[lane] = fm < fp ? fm : fp;
        if (tval) {
            tval[off + 2 * lane] = ap;
            tval[off + 2 * lane + 1] = am;
        }
    }
    __syncthreads();
    // ranking by counting: (w, position in I) ascending -- positions are in the order of the dimensions
    if (lane < nI) {
        const double wi = sW[lane];
        int rank = 0;
        for (int j = 0; j < nI; ++j) rank += (sW[j] < wi || (sW[j] == wi && j < lane)) ? 1 : 0;
        sRank[lane] = rank;
    }
    __syncthreads();
    // the children: centre = the sampled point, levels = the parent's + 1 on the dimensions of rank <= the child's
    for (int e = lane; e < 2 * nI * D; e += 64) {
        const int slot = e / D, d = e - slot * D, rho = sRank[slot >> 1];
        const size_t ch = (size_t)n0 + off + slot;
        st.c[ch * D + d] = st.x[(size_t)(off + slot) * D + d];
        const int up = sPos[d] >= 0 && sRank[sPos[d]] <= rho ? 1 : 0;
        st.lev[ch * D + d] = (unsigned char)(sLev[d] + up);
        if (d == 0) st.cls[ch] = s + rho + 1;
    }
    if (lane < D && sPos[lane] >= 0) st.lev[(size_t)r * D + lane] = (unsigned char)(k + 1);
    if (lane == 0) st.cls[r] = (k + 1) * D;
}

// the best rectangle from a merge of the final tables -> st.out; the flag word is reported and cleared; the trace's store
__global__ __launch_bounds__(WG) void dir_result_kernel(DirState st) {
    __shared__ unsigned long long sRedK[WG];
    __shared__ int sRedI[WG];
    const int tid = threadIdx.x, D = st.D, n = st.hdr[DIR_N_RECT], parts = (n + DIR_CHUNK - 1) / DIR_CHUNK;
    unsigned long long bk = DIR_KEY_EMPTY;
    int bi = DIR_IDX_EMPTY;
    for (int s = tid; s < st.n_cls; s += WG) {
        unsigned long long k;
        int i;
        dir_merge(st, parts, s, k, i);
        if (k < bk || (k == bk && i < bi)) {
            bk = k;
            bi = i;
        }
    }
    dir_block_min(sRedK, sRedI, bk, bi);
    for (int d = tid; d < D; d += WG) st.out[d] = st.c[(size_t)bi * D + d];
    if (tid == 0) {
        const double f = dir_unkey(bk);
        unsigned flags = (unsigned)st.hdr[DIR_STOP];
        if (flags == 0u) flags = st.hdr[DIR_EVALS] >= st.max_evals ? ROBO_DIRECT_STOP_BUDGET : ROBO_DIRECT_STOP_ITERS;
        flags |= *st.flags;
        *st.flags = 0u;
        st.out[D] = f == 0.0 ? 0.0 : -f;
        st.out[D + 1] = __longlong_as_double((long long)st.hdr[DIR_EVALS]);
        st.out[D + 2] = __longlong_as_double((long long)st.hdr[DIR_ITERS]);
        st.out[D + 3] = __longlong_as_double((long long)flags);
    }
    if (!st.trace) return;
    double* store = st.trace + (size_t)(st.T + 1) * dir_trace_row(D, st.B);
    const size_t w = (size_t)2 * D + 1;
    for (size_t e = tid; e < (size_t)st.cap * w; e += WG) {
        const size_t r = e / w, j = e - r * w;
        double v = 0.0;
        if (r < (size_t)n) v = j < (size_t)D ? st.c[r * D + j] : (j < 2 * (size_t)D ? (double)st.lev[r * D + j - D] : st.f[r]);
        store[e] = v;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
void dir_free(DirWork* w) {
    if (!w) return;
    hipFree(w->d_block);
    hipFree(w->d_trace);
    delete w;
}

int launch_dir_init(robo_ctx* ctx, const DirState& st) {
    hipLaunchKernelGGL(dir_init_kernel, dim3(1), dim3(WG), 0, ctx->stream, st);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_dir_classmin(robo_ctx* ctx, const DirState& st, int force) {
    const unsigned grid = (unsigned)((st.cap + DIR_CHUNK - 1) / DIR_CHUNK);
    hipLaunchKernelGGL(dir_classmin_kernel, dim3(grid), dim3(WG), 0, ctx->stream, st, force);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_dir_select(robo_ctx* ctx, const DirState& st, int t) {
    hipLaunchKernelGGL(dir_select_kernel, dim3(1), dim3(WG), 0, ctx->stream, st, t);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_dir_divide(robo_ctx* ctx, const DirState& st, int t) {
    hipLaunchKernelGGL(dir_divide_kernel, dim3(t == 0 ? 1u : (unsigned)(st.B / 2)), dim3(64), 0, ctx->stream, st, t);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_dir_result(robo_ctx* ctx, const DirState& st) {
    hipLaunchKernelGGL(dir_result_kernel, dim3(1), dim3(WG), 0, ctx->stream, st);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

}  // namespace robo
