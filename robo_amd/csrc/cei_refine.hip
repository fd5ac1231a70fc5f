// Gradient refinement of the constrained-EI maximum (robo_cei_refine_cand; the rule is stated in include/robo_hip.h, the
// driver is in api_cei.hip): the epilogue that turns the moments of C + 1 GPs and their gradients at a start's trial point
// into the constrained value, its gradient and the step decision.
//
//   per trial, per GP in the order constraint 1 .. C, objective:  scale_inputs, cross_grad_kernel, that GP's solve,
//   cei_refine_eval_kernel (one workgroup per start)
//
// A constraint's launch forms z_k = (t_k - m_k) / s_k, l_k = log Phi(z_k) and dl_k = (phi / Phi)(z_k) dz_k and adds them to
// the running L and dL, which live where the marginal refinement keeps its partial sums (RefineState fy, gy, bad): no array
// beyond refine.hip's state block.  The objective comes last, so its launch holds the finished L and dL next to its own
// factor: it combines them by cei_kernel's rule, decides and writes the next trial.  Without a feasible incumbent
// (has_eta = 0) the driver launches no objective epilogue (its GP is not solved at all) and the last constraint decides.
// The dot products, the moments, the objective's formulas and the decision are refine_eval.h's, shared with
// refine_eval_kernel: with C = 0 and has_eta = 1 this kernel executes refine_eval_kernel's operations for one sample.
#include "common.h"
#include "kern_math.h"
#include "refine_eval.h"

namespace robo {

__global__ __launch_bounds__(256) void cei_refine_eval_kernel(RefineState st, const double* __restrict__ V, int ldv,
                                                              int ncols, const double* __restrict__ q,
                                                              const double* __restrict__ mu, const double* __restrict__ ism,
                                                              CovParams cp, double mean_c, double y_mean, double y_std,
                                                              CeiRefineStep step, int t, int T) {
    __shared__ double sdot[MAX_DIM];
    __shared__ double sgp[MAX_DIM];
    const int k = blockIdx.x, D = cp.dim, tid = threadIdx.x;
    const RefineCarried c = refine_carried(st, k, D, tid, !step.first);
    const RefineMoments p = refine_moments(st, k, tid, c.mine, V, ldv, ncols, q, mu, ism, cp, mean_c, y_mean, y_std, sdot);
    double L = c.facc0, dL = c.gacc0;          // (0 in the first launch of a trial)
    const int bad = c.bad0 | (p.floored ? 1 : 0);
    if (!step.objective) {
        const double z = rn_div(rn_sub(step.thr, p.m), p.sd);
        const double dz = (-p.dm - z * p.ds) / p.sd;
        const double dl = pdf_over_cdf(z) * dz;
        L = rn_add(L, norm_logcdf(z));
        dL = step.first ? dl : dL + dl;
        if (!step.last) {          // more GPs to come: leave the partial sums behind
            if (c.mine) st.gy[c.kd] = dL;
            if (tid == 0) {
                st.fy[k] = L;
                st.bad[k] = bad;
            }
            return;
        }
    }
    const bool log_form = step.kind == ROBO_ACQ_LOG_EI;
    double fy, gyd;
    if (step.objective && step.has_eta) {
        double f0, g0;
        refine_acq(step.kind, step.par, step.eta, p, &f0, &g0);
        if (step.C == 0) {         // the plain value itself, not a product with exp(0)
            fy = f0;
            gyd = g0;
        } else if (log_form) {
            fy = rn_add(f0, L);
            gyd = g0 + dL;
        } else {
            const double P = exp(L);
            fy = rn_mul(f0, P);
            gyd = P * (g0 + f0 * dL);
        }
    } else if (log_form) {
        fy = L;
        gyd = dL;
    } else {
        const double P = exp(L);
        fy = P;
        gyd = P * dL;
    }
    refine_step(st, k, tid, D, c, fy, gyd, bad, t, T, sgp);
}

int launch_cei_refine_eval(robo_gp* gp, const RefineState& st, const robo_cand* ws, const CeiRefineStep& step, int t, int T) {
    const int ncols = (gp->n + NB - 1) / NB * NB;        // the block rows the solve touched
    hipLaunchKernelGGL(cei_refine_eval_kernel, dim3((unsigned)st.K), dim3(256), 0, gp->ctx->stream, st,
                       (const double*)ws->d_V, gp->n_pad, ncols, (const double*)ws->d_q, (const double*)ws->d_mu,
                       (const double*)gp->d_theta, gp->cov, gp->mean_c, gp->y_mean, gp->y_std, step, t, T);
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

}  // namespace robo
