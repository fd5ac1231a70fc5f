// Knowledge gradient over a discretisation (Frazier, Powell & Dayanik 2009, stated for minimisation; no counterpart in
// the reference): KG(x) = min_j a_j - E_Z[ min_j (a_j + b_j Z) ] over n <= 65 lines per candidate, in the envelope form
// of include/robo_hip.h -- every term of the sum is non-negative, nothing of size |a| is ever subtracted.
//
//   sweep (predict.hip) + signed cross-covariance (infogain.hip cross_cov_kernel<TM, false>) -> d_S, d_var, d_mean
//   -> kg_kernel: lines (A, B) = (-a, -b) -> rank-counting sort by (B ascending, A descending, index ascending), equal
//      slopes keep their first line -> upper-envelope stack scan -> one term per lane -> the sum in ascending order
//   -> the sweep's own reduction (launch_argmax, acq.hip)
//
// One wavefront per candidate, four candidates per workgroup; a candidate's lines, its sorted lines and the stack live
// in that wave's slice of LDS (stride 66 doubles: lanes read consecutive doubles or one broadcast address, no bank
// conflicts).  The sort, the scan and the sum have a fixed order: the same candidate gives the same bits at any batch
// position and on any call.
#include "common.h"
#include "kern_math.h"

namespace robo {

constexpr int KG_WAVES = 4;      // candidates per workgroup
constexpr int KG_LD = 66;        // doubles per wave and LDS array (65 lines)

__device__ __forceinline__ double kg_nan() { return __longlong_as_double(0x7FF8000000000000LL); }

// mode 1: acq_sum[c] = KG   (the only or first hyper-parameter sample)
// mode 2: acq_sum[c] += KG  (next samples; fixed sample order, as acq_kernel)
__global__ __launch_bounds__(64 * KG_WAVES) void kg_kernel(const double* __restrict__ S, const double* __restrict__ var,
                                                           const double* __restrict__ mean,
                                                           const double* __restrict__ disc, long long m, int nb,
                                                           double sn2, int include_self, int mode,
                                                           double* __restrict__ acq_sum, unsigned* __restrict__ flags,
                                                           double* __restrict__ trace) {
    // lA / lB: the lines as read, later the stack's breakpoints / the terms; sA / sB: the lines in order
    __shared__ double lA[KG_WAVES][KG_LD], lB[KG_WAVES][KG_LD], sA[KG_WAVES][KG_LD], sB[KG_WAVES][KG_LD];
    __shared__ int sKeep[KG_WAVES][KG_LD], sStk[KG_WAVES][KG_LD], sTop[KG_WAVES];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long c = (long long)blockIdx.x * KG_WAVES + w;
    const bool live = c < m;                  // wave-uniform; every work-item reaches every barrier
    const int n = nb + (include_self ? 1 : 0);
    bool bad = false;
    if (live) {
        const double v = var[c], mu = mean[c];
        const double sigt = sqrt(v + sn2);
        if (lane < nb) {
            const double s = S[(size_t)c * NB + lane], a = disc[lane];
            const double b = s / sigt;
            lA[w][lane] = -a;
            lB[w][lane] = -b;
            bad = isnan(s) || isnan(a) || isnan(b);
            if (trace) trace[(size_t)c * (nb + 2) + lane] = s;
        }
        if (lane == 0) {
            const double b = v / sigt;
            bad = bad || isnan(v) || isnan(mu) || isnan(b);
            if (include_self) {
                lA[w][nb] = -mu;
                lB[w][nb] = -b;
            }
            if (trace) {
                trace[(size_t)c * (nb + 2) + nb] = v;
                trace[(size_t)c * (nb + 2) + nb + 1] = mu;
            }
        }
    }
    const bool any_bad = __ballot(bad) != 0ull;
    __syncthreads();
    // rank counting: line i goes to the number of lines that precede it; a line with an equal slope before it is dropped
    // (the second pass is line 64 alone)
    if (live)
        for (int i = lane; i < n; i += 64) {
            const double Ai = lA[w][i], Bi = lB[w][i];
            int rank = 0, dup = 0;
            for (int k = 0; k < n; ++k) {
                const double Ak = lA[w][k], Bk = lB[w][k];
                if (Bk < Bi) {
                    ++rank;
                } else if (Bk == Bi && (Ak > Ai || (Ak == Ai && k < i))) {
                    ++rank;
                    dup = 1;
                }
            }
            sA[w][rank] = Ai;
            sB[w][rank] = Bi;
            sKeep[w][rank] = !dup;
        }
    __syncthreads();
    // upper envelope of A + B z: the stack holds (line, breakpoint from which it is the maximum); the bottom's is -inf
    if (lane == 0) {
        int top = -1;
        if (live && !any_bad)
            for (int i = 0; i < n; ++i) {
                if (!sKeep[w][i]) continue;
                const double Ai = sA[w][i], Bi = sB[w][i];
                double cb = -__builtin_huge_val();
                while (top >= 0) {
                    const int t = sStk[w][top];
                    cb = (sA[w][t] - Ai) / (Bi - sB[w][t]);
                    if (!(cb <= lA[w][top])) break;
                    --top;
                    cb = -__builtin_huge_val();
                }
                ++top;
                sStk[w][top] = i;
                lA[w][top] = cb;
            }
        sTop[w] = top;
    }
    __syncthreads();
    const int top = sTop[w];
    if (lane + 1 <= top) {
        const int p = lane + 1;
        lB[w][p] = (sB[w][sStk[w][p]] - sB[w][sStk[w][p - 1]]) * norm_tail_mean(fabs(lA[w][p]));
    }
    __syncthreads();
    if (lane != 0 || !live) return;
    double kg = 0.0;
    for (int p = 1; p <= top; ++p) kg += lB[w][p];
    if (any_bad) kg = kg_nan();
    if (isnan(kg)) atomicOr(flags, (unsigned)ROBO_FLAG_NAN);
    if (mode == 1) acq_sum[c] = kg;
    else acq_sum[c] += kg;
}

int launch_kg(robo_ctx* ctx, const double* d_S, const double* d_var, const double* d_mean, const double* d_disc, int64_t m,
              int nb, double sn2, int include_self, bool first, double* d_acq_sum, unsigned* d_flags, double* d_trace) {
    hipLaunchKernelGGL(kg_kernel, dim3((unsigned)((m + KG_WAVES - 1) / KG_WAVES)), dim3(64 * KG_WAVES), 0, ctx->stream, d_S,
                       d_var, d_mean, d_disc, (long long)m, nb, sn2, include_self, first ? 1 : 2, d_acq_sum, d_flags,
                       d_trace);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

}  // namespace robo
