// The output transform of one candidate's posterior: post_kernel (predict.hip) and the acquisition screen's one-workgroup tail
// (acq.hip acq_tail_kernel) run the same statements, so the same bits come out.
#pragma once
#include "kern_math.h"

namespace robo {
__device__ __forceinline__ void post_point(double q, double mu, double x_last, const CovParams& cp, double mean_c, double y_mean,
                                           double y_std, double& m_out, double& v_out) {
    double m = mu + mean_c;
    double v = cov_self(cp, x_last) - q;
    m = m * y_std + y_mean;
    v = v * (y_std * y_std);
    const double eps = 2.220446049250313e-16;
    v = v < eps ? eps : v;   // np.clip(var, eps, inf); NaN propagates like np.clip
    m_out = m;
    v_out = v;
}
}  // namespace robo
