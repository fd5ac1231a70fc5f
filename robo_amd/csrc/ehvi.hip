// Two-objective expected hypervolume improvement over a sorted Pareto front (minimisation, independent posteriors; no
// counterpart in the reference), in the strip form of include/robo_hip.h:
//
//   EHVI = sum_{i=0}^{P} [ g(a_{i+1}; mu1, s1) - g(a_i; mu1, s1) ] g(b_i; mu2, s2),   g(b; mu, s) = s f((b - mu) / s),
//   f(z) = max(z, 0) + norm_tail_mean(|z|)   (the erfcx form of kern_math.h: exactly 0 beyond |z| = 36 on the left)
//
//   sweep of gp1 -> (mean1, var1) kept, sweep of gp2 (predict.hip) -> ehvi_kernel -> the sweep's own reduction
//   (launch_argmax, acq.hip)
//
// One lane per candidate.  The front index is uniform over the wavefront, so the front points are read through uniform
// loads: no LDS, no barrier.  A candidate's strips are summed in index order i = 0 .. P with the boundary value
// g(a_i) carried in a register, by a compensated sum; every operation of it is rounded once and never contracted (rn_*),
// so the same four moments give the same bits at any batch position, for any m and in either entry point.
#include "common.h"
#include "kern_math.h"

namespace robo {

constexpr int EHVI_WG = 64;      // one wavefront per workgroup: 65 536 candidates are four workgroups per CU

__device__ __forceinline__ double ehvi_nan() { return __longlong_as_double(0x7FF8000000000000LL); }

// g(b; mu, s) = E[(b - y)^+], y ~ N(mu, s^2); s == 0: max(b - mu, 0)
__device__ __forceinline__ double ehvi_g(double b, double mu, double s) {
    const double d = rn_sub(b, mu);
    if (s == 0.0) return fmax(d, 0.0);
    const double z = rn_div(d, s);
    return rn_mul(s, rn_add(fmax(z, 0.0), norm_tail_mean(fabs(z))));
}

__global__ __launch_bounds__(EHVI_WG) void ehvi_kernel(const double* __restrict__ mean1, const double* __restrict__ var1,
                                                       const double* __restrict__ mean2, const double* __restrict__ var2,
                                                       const double* __restrict__ front, int P, double r1, double r2,
                                                       long long m, double* __restrict__ out, unsigned* __restrict__ flags,
                                                       double* __restrict__ trace) {
    const long long c = (long long)blockIdx.x * EHVI_WG + threadIdx.x;
    const bool live = c < m;
    unsigned f = 0;
    if (live) {
        const double mu1 = mean1[c], v1 = var1[c], mu2 = mean2[c], v2 = var2[c];
        if (trace) {
            trace[(size_t)c * 4 + 0] = mu1;
            trace[(size_t)c * 4 + 1] = v1;
            trace[(size_t)c * 4 + 2] = mu2;
            trace[(size_t)c * 4 + 3] = v2;
        }
        const double s1 = sqrt(v1), s2 = sqrt(v2);
        // compensated (Kahan) sum: the accumulation costs 2 eps of the sum whatever P is, where the plain sum's bound grows
        // with P; four additions beside two evaluations of g per strip
        double acc = 0.0, comp = 0.0, glo = 0.0;           // g(a_0 = -inf) = 0
        for (int i = 0; i <= P; ++i) {
            const double ahi = i < P ? front[2 * i] : r1;           // a_{i+1}
            const double bi = i > 0 ? front[2 * i - 1] : r2;        // b_i
            const double ghi = ehvi_g(ahi, mu1, s1);
            // g increases with its first argument; the rounded values of two close front points may not: no negative strip
            const double d = rn_sub(ghi, glo), dg = d < 0.0 ? 0.0 : d;         // (a NaN stays)
            const double y = rn_sub(rn_mul(dg, ehvi_g(bi, mu2, s2)), comp);
            const double t = rn_add(acc, y);
            comp = rn_sub(rn_sub(t, acc), y);
            acc = t;
            glo = ghi;
        }
        if (isnan(mu1) || isnan(s1) || isnan(mu2) || isnan(s2)) acc = ehvi_nan();      // (s: a NaN or negative variance)
        if (s1 == 0.0 || s2 == 0.0) f |= ROBO_FLAG_ZERO_SIGMA;
        if (isnan(acc)) f |= ROBO_FLAG_NAN;
        out[c] = acc;
    }
    const unsigned long long any = __ballot(f != 0);
    if (any != 0ull && f != 0) atomicOr(flags, f);
}

int launch_ehvi(robo_ctx* ctx, const double* d_mean1, const double* d_var1, const double* d_mean2, const double* d_var2,
                const double* d_front, int P, double r1, double r2, int64_t m, double* d_out, unsigned* d_flags,
                double* d_trace) {
    hipLaunchKernelGGL(ehvi_kernel, dim3((unsigned)((m + EHVI_WG - 1) / EHVI_WG)), dim3(EHVI_WG), 0, ctx->stream, d_mean1,
                       d_var1, d_mean2, d_var2, d_front, P, r1, r2, (long long)m, d_out, d_flags, d_trace);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

}  // namespace robo
