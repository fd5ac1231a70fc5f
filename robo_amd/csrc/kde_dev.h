// Parzen estimators (kde.hip, api_kde.hip): the handle, what the host passes to the kernels and the ONE rule by which two
// partial log-sum-exps are joined.  The density is stated in include/robo_hip.h.
#pragma once
#include <cmath>

#include "common.h"

namespace robo {

constexpr int KDE_TC = 64;                      // candidates per workgroup of kde_sweep_kernel (16 per wave)
constexpr int KDE_CHUNK = 64;                   // components staged through LDS at a time (a multiple of 16)
constexpr int KDE_K2_SMALL = 32;                // the sweep's two LDS capacities: 2 D rounded up to 4 is at most this (D <= 16)
constexpr int KDE_K2_MAX = 2 * ROBO_KDE_MAX_DIM;   // ... or this
constexpr long long KDE_MAX_N = 1ll << 20;

inline int kde_k2(int D) { return (2 * D + 3) / 4 * 4; }         // length of a padded phi / psi row
inline int kde_npad(long long n) { return (int)((n + 15) / 16 * 16); }

// A partial log-sum-exp is a pair (mx, sm): the sum over its exponents e is  exp(mx) sm,  mx their maximum; the empty sum is
// (-inf, 0).  THE -inf RULE: joining with a part whose maximum is -inf (zero-weight or padding components only) leaves the
// other part's pair as it is -- no exp(-inf - -inf) is ever formed.  Otherwise the larger maximum is kept and the other
// side's sum is rescaled once.  `a` is the part that comes first in the fixed order; both the block update and the final
// combine of a candidate's four lane groups go through this one function.
struct KdeLse {
    double mx, sm;
};
__device__ __forceinline__ KdeLse kde_lse_join(const KdeLse a, const KdeLse b) {
    const double ninf = -INFINITY;
    if (b.mx == ninf) return a;
    if (a.mx == ninf) return b;
    KdeLse r;
    if (b.mx > a.mx) {
        r.mx = b.mx;
        r.sm = a.sm * exp(a.mx - b.mx) + b.sm;
    } else {
        r.mx = a.mx;
        r.sm = a.sm + b.sm * exp(b.mx - a.mx);
    }
    return r;
}
// the four exponents a lane holds of one 16 x 16 block, as a part of their own: components in ascending order
__device__ __forceinline__ KdeLse kde_lse_block(const v4d e) {
    KdeLse r;
    r.mx = fmax(fmax(e[0], e[1]), fmax(e[2], e[3]));
    r.sm = 0.0;
    if (r.mx == -INFINITY) return r;
    r.sm = (exp(e[0] - r.mx) + exp(e[1] - r.mx)) + (exp(e[2] - r.mx) + exp(e[3] - r.mx));
    return r;
}

struct KdeMixDev {                // one prepared mixture on the device
    const double* psi;            // npad x K2: [mu' / h^2 | 1 / h^2 | 0 ..]; padding components all 0
    const double* c;              // npad: c'; padding components -inf
    int npad;                     // a multiple of 16 (0: this mixture takes no part in the launch)
};

int launch_kde_prepare(robo_ctx* ctx, int D, const double* d_lo, const double* d_hi, const double* d_ctr, const double* d_mu,
                       const double* d_h, int shared_h, const double* d_w, double sum_w, long long n, double* d_psi, double* d_c);
// rows [0, m) through the mixtures whose npad is not 0: log l -> d_logl, log g -> d_logg, their difference -> d_ratio (when
// both ran); d_flags nullable
int launch_kde_sweep(robo_ctx* ctx, int D, const double* d_ctr, const KdeMixDev& good, const KdeMixDev& bad, const double* d_rows,
                     long long m, double* d_logl, double* d_logg, double* d_ratio, unsigned* d_flags);

}  // namespace robo

struct robo_kde {
    robo_ctx* ctx;
    int dim;
    double lo[ROBO_KDE_MAX_DIM], hi[ROBO_KDE_MAX_DIM];
    char* d_box;                  // [lo | hi | centre] (D each), one block (block_layout.h)
    double *d_lo, *d_hi, *d_ctr;
    struct Mix {
        bool set;
        long long n;
        int npad;
        char* d_block;            // [psi | c' | mu | h | w] laid out anew by every robo_kde_set_mixture (grows)
        size_t bytes;
        double *d_psi, *d_c, *d_mu, *d_h, *d_w;
    } mix[2];
    double* d_cand;               // the uploaded candidate rows (grows)
    size_t cand_cap;
    robo_cand* k;                 // log l (d_mean), log g (d_var), the ratio (d_acq_sum -> d_acq) and the argmax state of one m
};
