// What the expected-hypervolume kernels share (ehvi.hip: two objectives, strips; ehvi_box.hip: two to four objectives, boxes).
#pragma once
#include "common.h"
#include "kern_math.h"

namespace robo {

__device__ __forceinline__ double ehvi_nan() { return __longlong_as_double(0x7FF8000000000000LL); }

// g(b; mu, s) = E[(b - y)^+], y ~ N(mu, s^2); s == 0: max(b - mu, 0)
__device__ __forceinline__ double ehvi_g(double b, double mu, double s) {
    const double d = rn_sub(b, mu);
    if (s == 0.0) return fmax(d, 0.0);
    const double z = rn_div(d, s);
    return rn_mul(s, rn_add(fmax(z, 0.0), norm_tail_mean(fabs(z))));
}

}  // namespace robo
