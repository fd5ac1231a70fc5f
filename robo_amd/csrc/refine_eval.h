// What the epilogues of the gradient refinements share (refine.hip refine_eval_kernel, cei_refine.hip
// cei_refine_eval_kernel): one workgroup of 256 work-items per start; what a launch overwrites is read first
// (refine_carried), the posterior moments and their gradients at the trial point come from the solved pseudo-rows
// (refine_moments), the objective's value and gradient from them (refine_acq), and the launch that holds the finished
// value decides and writes the next trial (refine_step).  Device code only; the two kernels keep their own combination
// rule between these parts and nothing else.
#pragma once
#include "common.h"
#include "kern_math.h"

namespace robo {

// ---- Phi(z) / h(z), h = z Phi + phi: the factor of dz in d log EI ----------------------------------------------------------
// z >= -1: the plain quotient (h has no cancellation there).  z < -1, t = -z: with the Mills ratio
// M(t) = Phi(-t) / phi(t) = sqrt(pi / 2) erfcx(t / sqrt 2) the quotient is M / (1 - t M), free of underflow; 1 - t M
// ~ 1 / t^2 cancels and amplifies erfcx's rounding by t^2 (relative error ~ t^2 eps: 5.7e-14 at t = 16).  From t = 16 on
// the asymptotic series in u = 1 / t^2
//     t M = 1 - u + 3 u^2 - 15 u^3 + ...,      1 - t M = u (1 - 3 u + 15 u^2 - 105 u^3 + ...)
// is used with 12 terms: the first omitted term is 23!! u^12 = 4e-18 at t = 16 (below one ulp) and falls from there.
constexpr double REFINE_TAIL_T = 16.0;
__device__ __forceinline__ double cdf_over_h(double z) {
    if (z >= -1.0) {
        const double P = norm_cdf(z);
        return P / (z * P + norm_pdf(z));
    }
    const double t = -z;
    if (t < REFINE_TAIL_T) {
        const double M = 1.25331413731550025121 * erfcx(t * SQRT1_2);
        return M / (1.0 - t * M);
    }
    const double u = 1.0 / (t * t);
    double num = 0.0, den = 0.0;       // Horner from the highest term: coefficients (-1)^n (2n - 1)!! and (-1)^n (2n + 1)!!
    double c = 316234143225.0;         // 23!!
    for (int n = 12; n >= 1; --n) {    // c = (2n - 1)!! on entry
        const double sgn = (n & 1) ? -1.0 : 1.0;
        num = (num + sgn * c) * u;
        den = (den + sgn * c * (double)(2 * n + 1)) * u;
        c /= (double)(2 * n - 1);
    }
    // t M = 1 + num,  (1 - t M) / u = 1 + den  ->  M / (1 - t M) = t (1 + num) / (1 + den)
    return t * (1.0 + num) / (1.0 + den);
}

// ---- phi(z) / Phi(z): the factor of dz in d log Phi -------------------------------------------------------------------------
// z >= -1: the plain quotient (Phi >= 0.158; phi underflows to 0 on the far right, where the ratio is 0 to every digit).
// z < -1: the reciprocal of the Mills ratio, 1 / (sqrt(pi / 2) erfcx(-z / sqrt 2)): no underflow where Phi has long
// vanished, so the gradient of log Phi stays finite wherever log Phi does.
__device__ __forceinline__ double pdf_over_cdf(double z) {
    if (z >= -1.0) return norm_pdf(z) / norm_cdf(z);
    return 1.0 / (SQRT_PI_2 * erfcx(-z * SQRT1_2));
}

// ---- what a start carries into a launch ---------------------------------------------------------------------------------------
struct RefineCarried {
    long long start;
    int was_frozen, bad0;
    double fx, alpha0, aused, facc0;   // facc0 / gacc0 / bad0: the partial sums an earlier launch of this trial left (carry)
    bool mine;                         // this work-item owns dimension tid
    size_t kd;
    double xd0, gd0, yd, gacc0;
};

__device__ __forceinline__ RefineCarried refine_carried(const RefineState& st, int k, int D, int tid, bool carry) {
    RefineCarried c;
    c.start = st.start[k];
    c.was_frozen = st.frozen[k];
    c.fx = st.f[k];
    c.alpha0 = st.alpha[k];
    c.aused = st.aused[k];
    c.facc0 = carry ? st.fy[k] : 0.0;
    c.bad0 = carry ? st.bad[k] : 0;
    c.mine = tid < D;
    c.kd = (size_t)k * D + (c.mine ? tid : 0);
    c.xd0 = st.x[c.kd];
    c.gd0 = st.g[c.kd];
    c.yd = st.y[c.kd];
    c.gacc0 = carry ? st.gy[c.kd] : 0.0;
    return c;
}

// ---- posterior moments and their gradients at start k's trial point ------------------------------------------------------------
// Rows (k E .. k E + D) of the solved workspace are v = L^-1 k_*(y_k) and w_d = L^-1 dk_*/dxs_d; q / mu are the solve's
// reductions |row|^2 and row . z.  The D dot products v . w_d over the N columns are the memory-bound part: wave w takes
// the rows d = w, w + 4, ..., every lane two adjacent columns per load (16 B), so each w_d row is requested once and v (one
// row, reused D times by the four waves) is expected to come from the cache -- by construction, not measured; with one
// workgroup per start and two FMA chains per lane the kernel is more likely bound by load latency than by bandwidth
// (its measured share of an iteration is in NOTES.md "Gradient refinement on the device").  Then m, v, dm, dv as
// predgrad_post_kernel forms them (every work-item: a few dozen flops; dm, dv, ds are this work-item's components, 0
// beyond D).  sdot: MAX_DIM doubles of LDS.  Holds a barrier: every work-item of the workgroup calls it.
struct RefineMoments {
    double m, v, sd, dm, dv, ds;
    bool floored;                      // the variance sat below DBL_EPSILON and was raised to it
};

__device__ __forceinline__ RefineMoments refine_moments(const RefineState& st, int k, int tid, bool mine,
                                                        const double* __restrict__ V, int ldv, int ncols,
                                                        const double* __restrict__ q, const double* __restrict__ mu,
                                                        const double* __restrict__ ism, const CovParams& cp, double mean_c,
                                                        double y_mean, double y_std, double* sdot) {
    const int D = cp.dim, E = D + 1, lane = tid & 63, wave = tid >> 6;
    const double* v0 = V + (size_t)k * E * ldv;
    for (int d = wave; d < D; d += 4) {
        const double* vd = v0 + (size_t)(1 + d) * ldv;
        double a0 = 0.0, a1 = 0.0;
        for (int j = 2 * lane; j < ncols; j += 128) {
            const double2 a = *reinterpret_cast<const double2*>(v0 + j);
            const double2 b = *reinterpret_cast<const double2*>(vd + j);
            a0 = fma(a.x, b.x, a0);
            a1 = fma(a.y, b.y, a1);
        }
        double acc = a0 + a1;
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) sdot[d] = acc;
    }
    __syncthreads();

    RefineMoments p;
    const double u = st.ys[(size_t)k * D + D - 1];
    p.m = (mu[(size_t)k * E] + mean_c) * y_std + y_mean;
    const double vraw = (cov_self(cp, u) - q[(size_t)k * E]) * (y_std * y_std);
    const double eps = 2.220446049250313e-16;
    p.floored = !(vraw >= eps);
    p.v = p.floored ? eps : vraw;
    p.sd = sqrt(p.v);
    p.dm = 0.0;
    p.dv = 0.0;
    if (mine) {
        const double dself = (cp.kind == ROBO_KERNEL_FABOLAS && tid == D - 1) ? 2.0 * cp.amp * cp.blr_b * u : 0.0;
        p.dm = mu[(size_t)k * E + 1 + tid] * ism[tid] * y_std;
        p.dv = (dself - 2.0 * sdot[tid]) * ism[tid] * (y_std * y_std);
    }
    p.ds = p.dv / (2.0 * p.sd);
    return p;
}

// ---- value and this work-item's gradient component of a closed-form acquisition from the moments ---------------------------------
__device__ __forceinline__ void refine_acq(int kind, double par, double eta, const RefineMoments& p, double* f_out,
                                           double* df_out) {
    const double m = p.m, v = p.v, sd = p.sd, dm = p.dm, ds = p.ds;
    double f, df;
    if (kind == ROBO_ACQ_LCB) {
        f = acq_lcb(m, v, par);
        df = -(dm - par * ds);
    } else {
        const double z = (eta - m - par) / sd;
        if (kind == ROBO_ACQ_EI) {
            f = acq_ei(m, v, eta, par);
            if (f < 0.0 && f > -2.2250738585072014e-308) f = 0.0;    // as acq_kernel
            df = -dm * norm_cdf(z) + ds * norm_pdf(z);
        } else if (kind == ROBO_ACQ_PI) {
            f = acq_pi(m, v, eta, par);
            df = -(norm_pdf(z) / sd) * (dm + ds * z);
        } else {
            f = acq_log_ei(m, v, eta, par);
            const double dz = (-dm - z * ds) / sd;
            df = ds / sd + cdf_over_h(z) * dz;
        }
    }
    *f_out = f;
    *df_out = df;
}

// ---- the decision on the finished value fy (gradient component gyd) of trial t, the trace row, the next trial point ---------------
// Identical in every work-item; the accept test, the step-length update, the trial point and its clip are single rn_*
// operations on stored doubles.  sgp: MAX_DIM doubles of LDS.  Holds a barrier: every work-item of the workgroup calls it.
__device__ __forceinline__ void refine_step(const RefineState& st, int k, int tid, int D, const RefineCarried& c, double fy,
                                            double gyd, int bad, int t, int T, double* sgp) {
    const double ninf = -__builtin_huge_val();
    const bool mine = c.mine;
    const size_t kd = c.kd;
    const bool trial_bad = bad != 0 || !isfinite(fy);
    int frozen = c.was_frozen, code;
    bool accept = false;
    double alpha = c.alpha0;
    if (c.start < 0) {
        code = 2;
    } else if (t == 0) {             // the start itself: always the current point
        accept = true;
        code = trial_bad ? 3 : 1;
        if (trial_bad) frozen = 1;
    } else if (c.was_frozen) {
        code = 2;
    } else if (trial_bad) {          // variance on its floor or value not finite: not taken, and the start stops here
        code = 3;
        frozen = 1;
    } else {
        accept = fy > c.fx;
        code = accept ? 1 : 0;
        alpha = accept ? fmin(rn_mul(2.0, c.alpha0), 0.5) : rn_mul(c.alpha0, 0.5);
    }
    const double xd = accept ? c.yd : c.xd0, gd = accept ? gyd : c.gd0;

    if (st.trace) {
        double* row = st.trace + ((size_t)t * st.K + k) * (2 * D + 3);
        if (mine) {
            row[tid] = c.yd;
            row[D + 1 + tid] = gyd;
        }
        if (tid == 0) {
            row[D] = fy;
            row[2 * D + 1] = c.aused;
            row[2 * D + 2] = (double)code;
        }
    }

    // next trial: projected direction of unit length, clipped to the box
    double gp = 0.0;
    if (mine) gp = ((xd <= 0.0 && gd < 0.0) || (xd >= 1.0 && gd > 0.0)) ? 0.0 : gd;
    if (mine) sgp[tid] = gp;
    __syncthreads();
    double n2 = 0.0;
    for (int d = 0; d < D; ++d) n2 += sgp[d] * sgp[d];
    const double nrm = sqrt(n2);
    const bool more = t < T;
    if (more && !frozen && !(nrm > 0.0 && isfinite(nrm))) frozen = 1;    // no ascent direction left inside the box
    if (mine) {
        double yn = xd;
        if (more && !frozen) {
            yn = rn_add(xd, rn_div(rn_mul(alpha, gp), nrm));
            yn = yn < 0.0 ? 0.0 : (yn > 1.0 ? 1.0 : yn);
        }
        st.y[kd] = yn;
        if (accept) {
            st.x[kd] = xd;
            st.g[kd] = gd;
        }
    }
    if (tid == 0) {
        if (accept) st.f[k] = fy;
        else if (c.start < 0) st.f[k] = ninf;
        st.alpha[k] = alpha;
        st.aused[k] = alpha;
        st.frozen[k] = frozen;
        if (frozen && !c.was_frozen) atomicOr(st.flags, ROBO_FLAG_FROZEN);
    }
}

}  // namespace robo
