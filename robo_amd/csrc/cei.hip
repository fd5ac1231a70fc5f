// Constrained expected improvement: EI weighted by the probability of feasibility under C black-box constraints with
// independent posteriors (Schonlau et al. 1998; Gardner et al. 2014; Gelbart et al. 2014; no counterpart in the reference),
// in the form of include/robo_hip.h:
//
//   z_k = (t_k - mu_k) / s_k,   L = sum_{k=1..C} norm_logcdf(z_k),   PoF = exp(L)
//   EI:  acq_ei(mu_0, var_0, eta, par) * PoF        LogEI:  acq_log_ei(mu_0, var_0, eta, par) + L
//   no feasible observation yet (has_eta == 0):  PoF resp. L alone
//
//   sweeps of the objective's and the constraints' GPs (predict.hip) -> rows of the handle's sample tables -> cei_kernel
//   -> the sweep's own reduction (launch_argmax, acq.hip)
//
// One lane per candidate.  The constraint index is uniform over the wavefront and the thresholds are kernel arguments, so a
// lane reads its own 2 (C + 1) moments (coalesced along the rows) and nothing else: no LDS, no barrier.  The objective factor
// is the plain sweep's (acq_ei / acq_log_ei of kern_math.h with acq_kernel's guards), the log-probabilities are summed in
// index order, and the rule's own operations are rounded once and never contracted (rn_*), so the same moments give the same
// bits at any batch position, for any m and in either entry point.
#include "common.h"
#include "kern_math.h"

namespace robo {

constexpr int CEI_WG = 64;       // one wavefront per workgroup, as ehvi.hip

__device__ __forceinline__ double cei_nan() { return __longlong_as_double(0x7FF8000000000000LL); }

__global__ __launch_bounds__(CEI_WG) void cei_kernel(const double* __restrict__ mean0, const double* __restrict__ var0,
                                                     const double* __restrict__ means, const double* __restrict__ vars,
                                                     long long stride, int C, CeiThresholds th, int kind, double par,
                                                     double eta, int has_eta, long long m, double* __restrict__ out,
                                                     unsigned* __restrict__ flags, double* __restrict__ trace) {
    const long long c = (long long)blockIdx.x * CEI_WG + threadIdx.x;
    unsigned f = 0;
    if (c < m) {
        const int width = 2 * (C + 1) + 2;
        double* tr = trace ? trace + (size_t)c * width : nullptr;
        const double mu0 = mean0[c], v0 = var0[c];
        if (tr) {
            tr[0] = mu0;
            tr[1] = v0;
        }
        bool nan = isnan(mu0) || isnan(sqrt(v0));               // (sqrt: a NaN or negative variance)
        double L = 0.0;
        for (int k = 0; k < C; ++k) {
            const double mu = means[(size_t)k * stride + c], v = vars[(size_t)k * stride + c];
            if (tr) {
                tr[2 * k + 2] = mu;
                tr[2 * k + 3] = v;
            }
            const double s = sqrt(v), t = th.t[k];
            double l;
            if (s == 0.0) {
                l = mu <= t ? 0.0 : -__builtin_huge_val();
                f |= ROBO_FLAG_ZERO_SIGMA;
            } else {
                l = norm_logcdf(rn_div(rn_sub(t, mu), s));
            }
            nan = nan || isnan(mu) || isnan(s);
            L = rn_add(L, l);
        }
        const bool log_form = kind == ROBO_ACQ_LOG_EI;
        double obj = log_form ? 0.0 : 1.0, a;
        if (has_eta) {
            if (log_form) {
                obj = acq_log_ei(mu0, v0, eta, par);
            } else {
                obj = acq_ei(mu0, v0, eta, par);
                if (obj < 0.0 && obj > -2.2250738585072014e-308) obj = 0.0;      // (acq_kernel's guard, acq.hip)
                if (obj < 0.0) f |= ROBO_FLAG_NEGATIVE_EI;
            }
            if (sqrt(v0) == 0.0) f |= ROBO_FLAG_ZERO_SIGMA;
            // C == 0: the plain sweep's value itself, not a product with exp(0)
            a = C == 0 ? obj : (log_form ? rn_add(obj, L) : rn_mul(obj, exp(L)));
        } else {
            a = log_form ? L : exp(L);
        }
        if (nan) a = cei_nan();
        if (isnan(a)) f |= ROBO_FLAG_NAN;
        if (tr) {
            tr[width - 2] = L;
            tr[width - 1] = obj;
        }
        out[c] = a;
    }
    const unsigned long long any = __ballot(f != 0);
    if (any != 0ull && f != 0) atomicOr(flags, f);
}

int launch_cei(robo_ctx* ctx, const double* d_mean0, const double* d_var0, const double* d_means, const double* d_vars,
               int64_t stride, int C, const CeiThresholds& th, int kind, double par, double eta, int has_eta, int64_t m,
               double* d_out, unsigned* d_flags, double* d_trace) {
    hipLaunchKernelGGL(cei_kernel, dim3((unsigned)((m + CEI_WG - 1) / CEI_WG)), dim3(CEI_WG), 0, ctx->stream, d_mean0, d_var0,
                       d_means, d_vars, (long long)stride, C, th, kind, par, eta, has_eta, (long long)m, d_out, d_flags,
                       d_trace);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

}  // namespace robo
