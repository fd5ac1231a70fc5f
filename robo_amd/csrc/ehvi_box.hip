// Expected hypervolume improvement for two to four objectives over a box decomposition of the non-dominated region
// (minimisation, independent posteriors; no counterpart in the reference), in the form of include/robo_hip.h:
//
//   EHVI = sum_{b=0}^{B-1} prod_{k=0}^{K-1} [ g(t_k[hi_bk]; mu_k, s_k) - g(t_k[lo_bk]; mu_k, s_k) ],   g = ehvi_g (ehvi_dev.h)
//
//   K sweeps (predict.hip) -> rows of the handle's sample tables -> ehvi_box_kernel -> the sweep's own reduction
//   (launch_argmax, acq.hip)
//
// The corners of the B boxes repeat the same sum_k n_k bound values, so a candidate's g is evaluated once per bound and
// the boxes only look it up.  A workgroup of EB_WG = 256 lanes takes a tile of EB_TC = 16 candidates:
//
//   table phase   G[row][c] = g(bounds[row]; mu_kc, s_kc) for every bound row (the objectives' bounds concatenated, as
//                 the caller passes them) and tile candidate c, in LDS, candidate-minor: entry e = row * 16 + c is filled
//                 by lane e mod 256, so a lane keeps its candidate.  The first row of an objective (-inf) stores +0.
//   box phase     lane = (c, l): candidate c = lane mod 16, box lane l = lane / 16 of EB_NL = 16.  The index pairs, one
//                 32-bit word (lo | hi << 16) per (box, objective), are staged EB_BC = 512 boxes at a time through LDS;
//                 the 16 lanes of one l read one word (a broadcast) and 16 consecutive doubles of a table row.  Box lane
//                 l takes the boxes b = l, l + 16, .. in ascending order: the K clipped differences, their product in
//                 objective order, a compensated (Kahan) sum.
//   combine       the 16 partial sums of a candidate through LDS, added in ascending l by the lane l = 0, compensated.
//
// Dynamic LDS: [mu 4 x 16 | s 4 x 16 | partials 16 x 16 | box words 512 x 4 | G rows x 16] = 11 264 + 128 rows bytes:
// 143 360 B at the limit of 4 x 258 rows (one workgroup per CU of gfx950's 160 KB), 36 KB for three objectives and a front
// of 64 points (four workgroups per CU).  No matrix instruction fits: the table phase is fp64 VALU (one erfcx per entry), the
// box phase LDS reads (2 K doubles and K words per box and candidate).
// Every operation of the rule is rounded once and never contracted (rn_*), and its order depends on nothing but
// (K, bounds, boxes, EB_NL): the same moments give the same bits at any batch position, for any m and in either entry point.
#include "ehvi_dev.h"

namespace robo {

constexpr int EB_TC = 16;        // candidates per workgroup
constexpr int EB_NL = 16;        // box lanes per candidate: part of the summation order
constexpr int EB_WG = EB_TC * EB_NL;
constexpr int EB_BC = 512;       // boxes staged per pass
constexpr int EB_HEAD = 2 * ROBO_EHVI_BOX_MAX_OBJ * EB_TC + EB_NL * EB_TC + EB_BC * ROBO_EHVI_BOX_MAX_OBJ / 2;   // doubles before G

__global__ __launch_bounds__(EB_WG) void ehvi_box_kernel(const double* __restrict__ mean, const double* __restrict__ var,
                                                         long long stride, EhviBoxShape sh,
                                                         const double* __restrict__ bounds,
                                                         const unsigned* __restrict__ boxes, int B, long long m,
                                                         double* __restrict__ out, unsigned* __restrict__ flags,
                                                         double* __restrict__ trace) {
    HIP_DYNAMIC_SHARED(double, sm)
    double* sMu = sm;                                          // [4][EB_TC]
    double* sS = sMu + ROBO_EHVI_BOX_MAX_OBJ * EB_TC;          // [4][EB_TC]
    double* sPart = sS + ROBO_EHVI_BOX_MAX_OBJ * EB_TC;        // [EB_NL][EB_TC]
    unsigned* sBox = reinterpret_cast<unsigned*>(sPart + EB_NL * EB_TC);      // [EB_BC][K]
    double* G = sm + EB_HEAD;                                  // [rows][EB_TC]
    const int K = sh.K, rows = sh.rows, b1 = sh.base[1], b2 = sh.base[2], b3 = sh.base[3];
    const int t = threadIdx.x, c = t & (EB_TC - 1), l = t / EB_TC;
    const long long cg = (long long)blockIdx.x * EB_TC + c;

    // the tile's moments; a lane past the batch computes on (0, 1) and writes nothing
    if (t < K * EB_TC) {
        const int k = l;
        const bool live = cg < m;
        const double mu = live ? mean[(size_t)k * stride + cg] : 0.0, v = live ? var[(size_t)k * stride + cg] : 1.0;
        if (trace && live) {
            trace[(size_t)cg * (2 * K) + 2 * k] = mu;
            trace[(size_t)cg * (2 * K) + 2 * k + 1] = v;
        }
        sMu[t] = mu;
        sS[t] = sqrt(v);
    }
    __syncthreads();

    // table phase: e mod EB_TC == c for every entry of this lane
    for (int e = t; e < rows * EB_TC; e += EB_WG) {
        const int row = e / EB_TC;
        const int k = (row >= b1) + (row >= b2) + (row >= b3);
        const int first = k == 0 ? 0 : (k == 1 ? b1 : (k == 2 ? b2 : b3));
        G[e] = row == first ? 0.0 : ehvi_g(bounds[row], sMu[k * EB_TC + c], sS[k * EB_TC + c]);
    }

    // box phase (the lanes of a last tile's candidates past m run it too, on their (0, 1) moments: the barriers stay uniform)
    double acc = 0.0, comp = 0.0;
    for (int cb = 0; cb < B; cb += EB_BC) {
        const int nb = B - cb < EB_BC ? B - cb : EB_BC;
        __syncthreads();                   // the table is complete; the previous pass's words are consumed
        for (int w = t; w < nb * K; w += EB_WG) sBox[w] = boxes[(size_t)cb * K + w];
        __syncthreads();
        for (int b = l; b < nb; b += EB_NL) {
            double p = 0.0;
            for (int k = 0; k < K; ++k) {
                const unsigned w = sBox[b * K + k];
                const int first = k == 0 ? 0 : (k == 1 ? b1 : (k == 2 ? b2 : b3));
                const double ghi = G[(first + (int)(w >> 16)) * EB_TC + c], glo = G[(first + (int)(w & 0xFFFFu)) * EB_TC + c];
                // g increases with its first argument; the rounded values of two close bounds may not: no negative factor
                const double d = rn_sub(ghi, glo), dg = d < 0.0 ? 0.0 : d;         // (a NaN stays)
                p = k == 0 ? dg : rn_mul(p, dg);
            }
            const double y = rn_sub(p, comp);
            const double s = rn_add(acc, y);
            comp = rn_sub(rn_sub(s, acc), y);
            acc = s;
        }
    }
    sPart[l * EB_TC + c] = acc;
    __syncthreads();

    unsigned f = 0;
    if (l == 0 && cg < m) {
        double tot = 0.0, cmp = 0.0;
        for (int j = 0; j < EB_NL; ++j) {
            const double y = rn_sub(sPart[j * EB_TC + c], cmp);
            const double s = rn_add(tot, y);
            cmp = rn_sub(rn_sub(s, tot), y);
            tot = s;
        }
        bool nan = false, zero = false;
        for (int k = 0; k < K; ++k) {
            const double mu = sMu[k * EB_TC + c], s = sS[k * EB_TC + c];
            nan = nan || isnan(mu) || isnan(s);             // (s: a NaN or negative variance)
            zero = zero || s == 0.0;
        }
        if (nan) tot = ehvi_nan();
        if (zero) f |= ROBO_FLAG_ZERO_SIGMA;
        if (isnan(tot)) f |= ROBO_FLAG_NAN;
        out[cg] = tot;
    }
    const unsigned long long any = __ballot(f != 0);       // (as ehvi_kernel: nothing for a clean wave, else the flagged lanes)
    if (any != 0ull && f != 0) atomicOr(flags, f);
}

int launch_ehvi_box(robo_ctx* ctx, const double* d_mean, const double* d_var, int64_t stride, const EhviBoxShape& sh,
                    const double* d_bounds, const unsigned* d_boxes, int B, int64_t m, double* d_out, unsigned* d_flags,
                    double* d_trace) {
    const size_t lds = ((size_t)EB_HEAD + (size_t)sh.rows * EB_TC) * sizeof(double);
    hipLaunchKernelGGL(ehvi_box_kernel, dim3((unsigned)((m + EB_TC - 1) / EB_TC)), dim3(EB_WG), lds, ctx->stream, d_mean,
                       d_var, (long long)stride, sh, d_bounds, d_boxes, B, (long long)m, d_out, d_flags, d_trace);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

}  // namespace robo
