// The regression forest's kernels (the rule is stated in include/robo_hip.h; DESIGN.md "Random forest on the device").
//   rf_presort_kernel  one workgroup per feature: a bitonic sort in LDS of (order-preserving key of x, row) pairs, once per
//                      fit and shared by every tree.
//   rf_grow_kernel     one workgroup per tree, the whole tree in one launch, level by level: the weights, the centred
//                      targets and each row's node id live in LDS; the tree's D feature lists live in memory, partitioned
//                      by node, so every node is one segment [start, start + cnt) of every list, sorted by that feature.
//                      A level is segmented scans over those lists (rf_tile_scan) and nothing else: no sort, no atomics on
//                      doubles, and the order of every sum is fixed by the list positions alone.
//   rf_sweep_kernel    a candidate per lane, its coordinates in LDS; the trees in tree order, a tree's nodes staged into LDS
//                      when they fit and read through L2 when they do not; Welford's update in tree order.
#include "forest_dev.h"
#include "philox.h"

namespace robo {

// ---- the presort ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long rf_key(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x + 0.0);      // (-0 sorts as +0)
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__global__ __launch_bounds__(WG) void rf_presort_kernel(const double* __restrict__ xt, int n, int P,
                                                        unsigned short* __restrict__ order) {
    __shared__ unsigned long long s_key[RF_MAX_N];
    __shared__ unsigned short s_row[RF_MAX_N];
    const int tid = threadIdx.x, f = blockIdx.x;
    for (int i = tid; i < P; i += WG) {
        s_key[i] = i < n ? rf_key(xt[(size_t)f * n + i]) : ~0ull;       // the padding sorts behind every row
        s_row[i] = (unsigned short)(i < n ? i : 0xFFFF);
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += WG) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long ki = s_key[i], kl = s_key[l];
                    const unsigned short ri = s_row[i], rl = s_row[l];
                    const bool gt = ki > kl || (ki == kl && ri > rl);
                    if (gt == ((i & k) == 0)) {
                        s_key[i] = kl; s_key[l] = ki;
                        s_row[i] = rl; s_row[l] = ri;
                    }
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < n; i += WG) order[(size_t)f * n + i] = s_row[i];
}

// ---- the segmented scan of one tile of WG list positions -------------------------------------------------------------------------
struct RfPair {
    double a, b;
};
constexpr int RF_SUM = 0, RF_BEST = 1;       // (a, b) += ;  the larger a, the earlier one on a tie

template <int OP>
__device__ __forceinline__ RfPair rf_combine(RfPair prev, RfPair cur) {
    if (OP == RF_SUM) return RfPair{prev.a + cur.a, prev.b + cur.b};
    return cur.a > prev.a ? cur : prev;
}

// Inclusive scan of v over the tile's positions, restarting at every head; `carry` is the running value that enters the tile
// and leaves it.  The combination tree -- shuffles inside a wave, the waves' totals in wave order, the carry in front -- is a
// function of the position alone.  s_tot / s_hd: 2 x 4 entries, `parity` alternates between consecutive calls.
template <int OP>
__device__ __forceinline__ RfPair rf_tile_scan(RfPair v, bool head, RfPair& carry, RfPair* s_tot, int* s_hd, int parity) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int h = head;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        RfPair o;
        o.a = __shfl_up(v.a, d);
        o.b = __shfl_up(v.b, d);
        const int oh = __shfl_up(h, d);
        if (lane >= d && !h) {
            v = rf_combine<OP>(o, v);
            h = oh;
        }
    }
    if (lane == 63) {
        s_tot[parity * 4 + wave] = v;
        s_hd[parity * 4 + wave] = h;
    }
    __syncthreads();
    RfPair c = carry, mine = carry;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w == wave) mine = c;
        c = s_hd[parity * 4 + w] ? s_tot[parity * 4 + w] : rf_combine<OP>(c, s_tot[parity * 4 + w]);
    }
    carry = c;
    return h ? v : rf_combine<OP>(mine, v);
}

// max_features of the D features without replacement: a partial Fisher-Yates shuffle, draw i from counter (node, i, tree, tag)
__device__ inline unsigned long long rf_draw_mask(unsigned long long seed, int tree, int node, int D, int mf) {
    if (mf >= D) return D == 64 ? ~0ull : ((1ull << D) - 1);
    unsigned char perm[64];
    for (int i = 0; i < D; ++i) perm[i] = (unsigned char)i;
    unsigned long long mask = 0;
    for (int i = 0; i < mf; ++i) {
        unsigned c[4] = {(unsigned)node, (unsigned)i, (unsigned)tree, 0x52460001u};
        double ua, ub;
        philox_uniform2(c, seed, ua, ub);
        int j = i + (int)(ua * (double)(D - i));
        if (j > D - 1) j = D - 1;
        const unsigned char p = perm[j];
        perm[j] = perm[i];
        perm[i] = p;
        mask |= 1ull << p;
    }
    return mask;
}

// ---- growing -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void rf_grow_kernel(RfGrow g) {
#pragma clang fp contract(off)
    __shared__ double s_yc[RF_MAX_N];
    __shared__ unsigned s_w[RF_MAX_N];
    __shared__ unsigned short s_nid[RF_MAX_N];
    __shared__ RfPair s_tot[8];
    __shared__ int s_hd[8];
    __shared__ unsigned s_union[2];
    __shared__ int s_count;
    const int tid = threadIdx.x, t = blockIdx.x, n = g.n, D = g.D;
    const size_t list_len = (size_t)D * n;
    unsigned short* cur = g.lists + (size_t)t * list_len;
    unsigned short* nxt = g.lists + ((size_t)g.T + t) * list_len;
    robo_rf_node* nodes = g.nodes + (size_t)t * g.stride;
    RfScratch* scr = g.scr + (size_t)t * g.stride;
    int parity = 0;

    // the weights, the centred targets, every row in the root
    for (int i = tid; i < n; i += WG) {
        s_w[i] = g.bootstrap ? 0u : 1u;
        s_yc[i] = g.y[i] - g.ybar;
        s_nid[i] = 0;
    }
    __syncthreads();
    if (g.bootstrap) {
        for (int j = tid; j < g.n_points; j += WG) {
            int r;
            if (g.idx) {
                r = g.idx[(size_t)t * g.n_points + j];
            } else {
                unsigned c[4] = {(unsigned)j, 0u, (unsigned)t, 0x52460000u};
                double ua, ub;
                philox_uniform2(c, g.seed, ua, ub);
                r = (int)(ua * (double)n);
                if (r > n - 1) r = n - 1;
            }
            atomicAdd(&s_w[r], 1u);
        }
        __syncthreads();
    }

    // the tree's lists: every feature's presorted rows without those of weight 0
    const int tiles_n = (n + WG - 1) / WG;
    int nt = 0;
    for (int f = 0; f < D; ++f) {
        RfPair carry = {0.0, 0.0};
        for (int tile = 0; tile < tiles_n; ++tile) {
            const int p = tile * WG + tid;
            const int r = p < n ? g.order[(size_t)f * n + p] : 0;
            const bool in = p < n && s_w[r] > 0;
            const RfPair v = rf_tile_scan<RF_SUM>(RfPair{in ? 1.0 : 0.0, 0.0}, p == 0, carry, s_tot, s_hd, parity);
            parity ^= 1;
            if (in) cur[(size_t)f * n + (int)v.a - 1] = (unsigned short)r;
        }
        nt = (int)carry.a;
    }
    if (tid == 0) {
        robo_rf_node& nd = nodes[0];
        nd.depth = 0;
        scr[0].start = 0;
        scr[0].cnt = nt;
        s_count = 1;
    }
    __syncthreads();
    const int tiles = (nt + WG - 1) / WG;

    int lvl0 = 0, lvl1 = 1;
    while (lvl0 < lvl1) {
        // (a) the frontier's statistics along list 0: W and S = sum w y_c, then M2 = sum w (y_c - S / W)^2
        for (int pass = 0; pass < 2; ++pass) {
            RfPair carry = {0.0, 0.0};
            for (int tile = 0; tile < tiles; ++tile) {
                const int p = tile * WG + tid;
                const bool in = p < nt;
                const int r = in ? cur[p] : 0, node = s_nid[r];
                const bool head = !in || p == 0 || s_nid[cur[p - 1]] != node;
                const bool last = in && (p == nt - 1 || s_nid[cur[p + 1]] != node);
                const double w = in ? (double)s_w[r] : 0.0;
                RfPair v;
                if (pass == 0) {
                    v = RfPair{w, w * s_yc[r]};
                } else {
                    const double d = in && node >= lvl0 ? s_yc[r] - scr[node].S / nodes[node].weight : 0.0;
                    v = RfPair{w * (d * d), 0.0};
                }
                v = rf_tile_scan<RF_SUM>(v, head, carry, s_tot, s_hd, parity);
                parity ^= 1;
                if (last && node >= lvl0) {
                    if (pass == 0) {
                        nodes[node].weight = v.a;
                        scr[node].S = v.b;
                    } else {
                        nodes[node].var = v.a / nodes[node].weight;
                        nodes[node].mean = scr[node].S / nodes[node].weight + g.ybar;
                    }
                }
            }
            __syncthreads();
        }
        // (b) the stop rules that need no split search, and the candidate features of the nodes that go on
        if (tid < 2) s_union[tid] = 0;
        __syncthreads();
        for (int node = lvl0 + tid; node < lvl1; node += WG) {
            robo_rf_node& nd = nodes[node];
            const bool stop = nd.weight < (double)g.min_split || nd.depth >= g.max_depth || nd.var <= g.eps_purity;
            nd.feature = -1;
            nd.left = nd.right = -1;
            nd.threshold = 0.0;
            nd.mask = stop ? 0ull : rf_draw_mask(g.seed, t, node, D, g.max_features);
            scr[node].best = -1.0;
            if ((unsigned)nd.mask) atomicOr(&s_union[0], (unsigned)nd.mask);
            if ((unsigned)(nd.mask >> 32)) atomicOr(&s_union[1], (unsigned)(nd.mask >> 32));
        }
        __syncthreads();
        const unsigned long long uni = (unsigned long long)s_union[1] << 32 | s_union[0];
        // (c) one pass per candidate feature: the prefix (W_L, S_L) at every position, the score at every admissible
        // boundary, the best of each segment under the tie rule
        for (int f = 0; f < D; ++f) {
            if (!(uni >> f & 1)) continue;
            const unsigned short* lf = cur + (size_t)f * n;
            const double* xf = g.xt + (size_t)f * n;
            RfPair carry = {0.0, 0.0}, bcarry = {-1.0, 0.0};
            for (int tile = 0; tile < tiles; ++tile) {
                const int p = tile * WG + tid;
                const bool in = p < nt;
                const int r = in ? lf[p] : 0, node = s_nid[r];
                const int r2 = in && p + 1 < nt ? lf[p + 1] : r;
                const bool head = !in || p == 0 || s_nid[lf[p - 1]] != node;
                const bool last = in && (p == nt - 1 || s_nid[r2] != node);
                const double w = in ? (double)s_w[r] : 0.0;
                const RfPair v = rf_tile_scan<RF_SUM>(RfPair{w, w * s_yc[r]}, head, carry, s_tot, s_hd, parity);
                parity ^= 1;
                RfPair b = {-1.0, 0.0};
                const bool search = in && node >= lvl0 && (nodes[node].mask >> f & 1);
                if (search && !last && xf[r] != xf[r2]) {
                    const double WL = v.a, WR = nodes[node].weight - WL;
                    if (WL >= (double)g.min_leaf && WR >= (double)g.min_leaf) {
                        const double SL = v.b, SR = scr[node].S - SL;
                        b.a = (SL * SL) / WL + (SR * SR) / WR;
                        b.b = (double)(p - scr[node].start);
                    }
                }
                b = rf_tile_scan<RF_BEST>(b, head, bcarry, s_tot, s_hd, parity);
                parity ^= 1;
                if (search && last && b.a > scr[node].best) {       // (strictly: the lower feature keeps a tie)
                    scr[node].best = b.a;
                    scr[node].bfeat = f;
                    scr[node].bpos = (int)b.b;
                }
            }
            __syncthreads();
        }
        // (d) leaf or split; the children's ids from a scan over the frontier, in node order
        {
            RfPair carry = {0.0, 0.0};
            const int base = s_count;
            for (int n0 = lvl0; n0 < lvl1; n0 += WG) {
                const int node = n0 + tid;
                const bool split = node < lvl1 && nodes[node].mask != 0 && scr[node].best >= 0.0;
                const RfPair v = rf_tile_scan<RF_SUM>(RfPair{split ? 1.0 : 0.0, 0.0}, node == lvl0, carry, s_tot, s_hd, parity);
                parity ^= 1;
                if (split) {
                    robo_rf_node& nd = nodes[node];
                    const RfScratch sc = scr[node];
                    const unsigned short* lf = cur + (size_t)sc.bfeat * n;
                    const double xa = g.xt[(size_t)sc.bfeat * n + lf[sc.start + sc.bpos]];
                    const double xb = g.xt[(size_t)sc.bfeat * n + lf[sc.start + sc.bpos + 1]];
                    double thr = 0.5 * xa + 0.5 * xb;
                    if (!(thr >= xa && thr < xb)) thr = xa;
                    const int left = base + 2 * ((int)v.a - 1);
                    nd.feature = sc.bfeat;
                    nd.threshold = thr;
                    nd.left = left;
                    nd.right = left + 1;
                    nodes[left].depth = nodes[left + 1].depth = nd.depth + 1;
                    scr[left].start = sc.start;
                    scr[left].cnt = sc.bpos + 1;
                    scr[left + 1].start = sc.start + sc.bpos + 1;
                    scr[left + 1].cnt = sc.cnt - (sc.bpos + 1);
                }
            }
            __syncthreads();
            if (tid == 0) s_count = base + 2 * (int)carry.a;
        }
        // (e) every row's way, then every list partitioned stably segment by segment
        for (int i = tid; i < n; i += WG) {
            const int node = s_nid[i];
            if (s_w[i] > 0 && node >= lvl0 && nodes[node].feature >= 0) {
                const bool right = !(g.xt[(size_t)nodes[node].feature * n + i] <= nodes[node].threshold);
                s_nid[i] = (unsigned short)(node | RF_SPLIT_BIT | (right ? RF_RIGHT_BIT : 0));
            }
        }
        __syncthreads();
        const int count = s_count;
        if (count > lvl1) {
            for (int f = 0; f < D; ++f) {
                const unsigned short* lf = cur + (size_t)f * n;
                RfPair carry = {0.0, 0.0};
                for (int tile = 0; tile < tiles; ++tile) {
                    const int p = tile * WG + tid;
                    const bool in = p < nt;
                    const int r = in ? lf[p] : 0, code = s_nid[r], node = code & RF_NODE_BITS;
                    const bool head = !in || p == 0 || (s_nid[lf[p - 1]] & RF_NODE_BITS) != node;
                    const bool left = in && (code & RF_SPLIT_BIT) && !(code & RF_RIGHT_BIT);
                    const RfPair v = rf_tile_scan<RF_SUM>(RfPair{left ? 1.0 : 0.0, 0.0}, head, carry, s_tot, s_hd, parity);
                    parity ^= 1;
                    if (in) {
                        int q = p;
                        if (code & RF_SPLIT_BIT) {
                            const int start = scr[node].start, lefts = (int)v.a;
                            q = left ? start + lefts - 1 : start + scr[nodes[node].left].cnt + (p - start - lefts);
                        }
                        nxt[(size_t)f * n + q] = (unsigned short)r;
                    }
                }
            }
            __syncthreads();
            for (int i = tid; i < n; i += WG) {
                const int code = s_nid[i];
                if (code & RF_SPLIT_BIT) {
                    const int left = nodes[code & RF_NODE_BITS].left;
                    s_nid[i] = (unsigned short)(code & RF_RIGHT_BIT ? left + 1 : left);
                }
            }
            unsigned short* sw = cur;
            cur = nxt;
            nxt = sw;
        }
        __syncthreads();
        lvl0 = lvl1;
        lvl1 = count;
    }
    if (tid == 0) g.counts[t] = lvl1;
}

// ---- the sweep ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void rf_sweep_kernel(const robo_rf_node* __restrict__ nodes, const int* __restrict__ counts,
                                                      int stride, int T, int D, int total_variance,
                                                      const double* __restrict__ rows, long long m,
                                                      double* __restrict__ out_mean, double* __restrict__ out_var,
                                                      double* __restrict__ out_pt) {
#pragma clang fp contract(off)
    __shared__ double s_x[RF_STAGE_COORDS];
    __shared__ double s_thr[RF_STAGE_NODES], s_mean[RF_STAGE_NODES], s_var[RF_STAGE_NODES];
    __shared__ short s_feat[RF_STAGE_NODES];
    __shared__ unsigned short s_left[RF_STAGE_NODES], s_right[RF_STAGE_NODES];
    const int tid = threadIdx.x, TC = blockDim.x, LD = D | 1;
    const long long row0 = (long long)blockIdx.x * TC, row = row0 + tid;
    const long long have = m - row0 < TC ? m - row0 : TC;
    for (long long e = tid; e < have * D; e += TC) {                  // (coalesced in memory, one row per lane in LDS)
        const int r = (int)(e / D), d = (int)(e - (long long)r * D);
        s_x[r * LD + d] = rows[(size_t)row0 * D + e];
    }
    __syncthreads();
    const double* x = s_x + tid * LD;
    bool bad = false;
    if (row < m)
        for (int d = 0; d < D; ++d) bad = bad || x[d] != x[d];
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    double mean = 0.0, M2 = 0.0, vsum = 0.0;
    for (int t = 0; t < T; ++t) {
        const robo_rf_node* tn = nodes + (size_t)t * stride;
        const int count = counts[t];
        const bool staged = count <= RF_STAGE_NODES;
        if (staged) {
            __syncthreads();                                           // (the walks of the tree before are over)
            for (int e = tid; e < count; e += TC) {
                const robo_rf_node nd = tn[e];
                s_thr[e] = nd.threshold;
                s_mean[e] = nd.mean;
                s_var[e] = nd.var;
                s_feat[e] = (short)nd.feature;
                s_left[e] = (unsigned short)nd.left;
                s_right[e] = (unsigned short)nd.right;
            }
            __syncthreads();
        }
        if (row < m) {
            int i = 0;
            double mu, v;
            if (staged) {
                for (int f = s_feat[i]; f >= 0; f = s_feat[i]) i = x[f] <= s_thr[i] ? s_left[i] : s_right[i];
                mu = s_mean[i];
                v = s_var[i];
            } else {
                for (int f = tn[i].feature; f >= 0; f = tn[i].feature) i = x[f] <= tn[i].threshold ? tn[i].left : tn[i].right;
                mu = tn[i].mean;
                v = tn[i].var;
            }
            const double d = mu - mean;
            mean = mean + d / (double)(t + 1);
            M2 = M2 + d * (mu - mean);
            vsum = vsum + v;
            if (out_pt) out_pt[(size_t)t * m + row] = bad ? nan : mu;
        }
    }
    if (row < m) {
        double var = M2 / (double)T;
        if (total_variance) var = vsum / (double)T + var;
        var = var < BLR_EPS ? BLR_EPS : var;
        out_mean[row] = bad ? nan : mean;
        out_var[row] = bad ? nan : var;
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
int launch_rf_presort(robo_ctx* ctx, const double* d_xt, int n, int D, unsigned short* d_order) {
    int P = 1;
    while (P < n) P <<= 1;
    hipLaunchKernelGGL(rf_presort_kernel, dim3(D), dim3(WG), 0, ctx->stream, d_xt, n, P, d_order);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_rf_grow(robo_ctx* ctx, const RfGrow& a) {
    hipLaunchKernelGGL(rf_grow_kernel, dim3(a.T), dim3(WG), 0, ctx->stream, a);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

int launch_rf_sweep(robo_ctx* ctx, const robo_rf_node* d_nodes, const int* d_counts, int stride, int T, int D,
                    int total_variance, const double* d_rows, long long m, double* d_mean, double* d_var,
                    double* d_per_tree) {
    const int TC = rf_sweep_tile(D);
    hipLaunchKernelGGL(rf_sweep_kernel, dim3((unsigned)((m + TC - 1) / TC)), dim3(TC), 0, ctx->stream, d_nodes, d_counts, stride,
                       T, D, total_variance, d_rows, m, d_mean, d_var, d_per_tree);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

}  // namespace robo
