// Expectation propagation for p_min and its derivatives (entropy search), batched over beliefs.
//
// Device restatement of robo_amd/util/epmgp.py (the reference's robo/util/epmgp.py:11-169): for a belief N(mu, Sigma)
// over nb representer points and every candidate minimiser k, nb - 1 Gaussian sites for the half-space factors
// "f_l >= f_k" are refined by moment matching until a sweep's summed site change is below 1e-3 (at most 50 sweeps);
// log Z_k and its derivatives follow in closed form from the final sites.  The nb problems of a belief are independent:
//   ep_site_kernel      one wave64 per (belief s, minimiser k): the sweeps on the working covariance V (row i in lane i,
//                       LDS), then the closed form (inner = I + R^T Sigma R from the INPUT Sigma, Cholesky with the jitter
//                       ladder for log det, LU with partial pivoting for inner^-1 as np.linalg.solve does)
//   ep_epilogue_kernel  one workgroup per belief: the -500 floor, log-sum-exp normalisation and the p_min-weighted
//                       corrections of the derivatives (the reference's element-wise Zm.T * Zm included, DESIGN.md
//                       "Mirrored quirks")
// Every operation of a sweep follows the host's order with contraction off, so device and host differ only through
// exp / log / erfc / sqrt.  No workgroup waits for another; the grid is exactly S x nb (S) workgroups.
#include "common.h"

namespace robo {

constexpr int EP_MAX = 64;       // nb cap (the representer batch of robo_ig_eval_cand)
constexpr int EP_LDA = 65;       // row stride of V / Sigma / G in LDS: odd, so a column read by 64 lanes is conflict-free
constexpr int EP_LDB = 63;       // row stride of inner (nb - 1 <= 63 rows)
constexpr double EP_SQRT2 = 1.4142135623730951;
constexpr double EP_EPS32 = 1.1920928955078125e-07;   // np.finfo(np.float32).eps
constexpr double EP_LOG_2PI = 1.8378770664093453;     // np.log(2.0) + np.log(np.pi)

// per-minimiser status (ep_site_kernel -> ep_epilogue_kernel): ROBO_OK, ROBO_NOT_POSITIVE_DEFINITE, ROBO_NUMERIC_ERROR

// Python's max(a, b): b if b > a else a (a NaN first argument is kept, a NaN second one is not)
__device__ __forceinline__ double py_max(double a, double b) { return b > a ? b : a; }

// inner = I + R^T Sigma R (+ jitter I) into B, from Sigma (sA) and the site precisions: column a of R is
// sqrt(p_a) (e_{l_a} - e_k) / sqrt(2), so (R^T Sigma)[a][j] = R_la Sigma[l_a][j] + R_ka Sigma[k][j]
__device__ void ep_build_inner(const double* sA, double* sB, const double* sRv, const double* sRk, int n, int k, double jitter) {
#pragma clang fp contract(off)
    const int a = threadIdx.x, m = n - 1;
    if (a < m) {
        const int la = a < k ? a : a + 1;
        const double ra = sRv[a], rka = sRk[a];
        const double tk = ra * sA[la * EP_LDA + k] + rka * sA[k * EP_LDA + k];
        for (int b = 0; b < m; ++b) {
            const int lb = b < k ? b : b + 1;
            const double tl = ra * sA[la * EP_LDA + lb] + rka * sA[k * EP_LDA + lb];
            double v = tl * sRv[b] + tk * sRk[b];
            v = (a == b ? 1.0 : 0.0) + v;
            if (a == b) v = v + jitter;
            sB[a * EP_LDB + b] = v;
        }
    }
    __syncthreads();
}

// in-place lower Cholesky of the m x m matrix in B (LAPACK dpotrf's failure rule: a pivot that is not > 0);
// diagonal of the factor -> sdiag.  Uniform result on every lane.
__device__ bool ep_cholesky(double* sB, double* sdiag, int m) {
    const int t = threadIdx.x;
    for (int c = 0; c < m; ++c) {
        const double d = sB[c * EP_LDB + c];
        if (!(d > 0.0)) return false;
        const double ljj = sqrt(d);
        if (t == 0) sdiag[c] = ljj;
        __syncthreads();          // every lane has read the pivot before row c's owner changes nothing, others update
        if (t > c && t < m) sB[t * EP_LDB + c] = sB[t * EP_LDB + c] / ljj;
        __syncthreads();
        if (t > c && t < m) {
            const double lt = sB[t * EP_LDB + c];
            for (int j = c + 1; j <= t; ++j) sB[t * EP_LDB + j] = sB[t * EP_LDB + j] - lt * sB[j * EP_LDB + c];
        }
        __syncthreads();
    }
    return true;
}

// in-place LU with partial pivoting (first largest |pivot|, as idamax) of the m x m matrix in B; false if singular
// (np.linalg.solve raises LinAlgError there)
__device__ bool ep_lu(double* sB, int* spiv, int m) {
    const int t = threadIdx.x;
    for (int c = 0; c < m; ++c) {
        int p = c;
        double best = fabs(sB[c * EP_LDB + c]);
        for (int r = c + 1; r < m; ++r) {
            const double v = fabs(sB[r * EP_LDB + c]);
            if (v > best) best = v, p = r;
        }
        if (!(best != 0.0)) return false;
        if (t == 0) spiv[c] = p;
        __syncthreads();
        if (p != c && t < m) {
            const double x = sB[c * EP_LDB + t];
            sB[c * EP_LDB + t] = sB[p * EP_LDB + t];
            sB[p * EP_LDB + t] = x;
        }
        __syncthreads();
        if (t > c && t < m) {
            const double l = sB[t * EP_LDB + c] / sB[c * EP_LDB + c];
            sB[t * EP_LDB + c] = l;
            for (int j = c + 1; j < m; ++j) sB[t * EP_LDB + j] = sB[t * EP_LDB + j] - l * sB[c * EP_LDB + j];
        }
        __syncthreads();
    }
    return true;
}

// grid: S * nb workgroups of 64 work-items, workgroup s * nb + k = (belief s, minimiser k)
__global__ __launch_bounds__(64) void ep_site_kernel(int nb, const double* __restrict__ mu_all,
                                                     const double* __restrict__ sigma_all, int with_deriv,
                                                     double* __restrict__ logz_all, double* __restrict__ dmu_all,
                                                     double* __restrict__ dmumu_all, double* __restrict__ ds_all,
                                                     int* __restrict__ sweeps_all, int* __restrict__ kstat_all) {
#pragma clang fp contract(off)
    __shared__ double sA[EP_MAX * EP_LDA];          // V during the sweeps; then Sigma; then G = inner^-1
    __shared__ double sB[(EP_MAX - 1) * EP_LDB];    // inner: Cholesky, then LU
    __shared__ double sM[EP_MAX], sVc[EP_MAX], sP[EP_MAX], sMP[EP_MAX], sLS[EP_MAX];
    __shared__ double sRv[EP_MAX], sRk[EP_MAX], sr[EP_MAX], sb[EP_MAX], sAb[EP_MAX], sxk[EP_MAX], srowk[EP_MAX],
        scolk[EP_MAX], sdiag[EP_MAX], su[EP_MAX];
    __shared__ int spiv[EP_MAX];
    __shared__ int snan;
    const int n = nb, t = threadIdx.x;
    const long long s = blockIdx.x / nb;
    const int k = (int)(blockIdx.x - s * nb);
    const long long pk = s * nb + k;
    const double* mu = mu_all + s * nb;
    const double* Sg = sigma_all + s * nb * nb;
    const int nt = n * (n + 1) / 2;

    for (int e = t; e < n * n; e += 64) sA[(e / n) * EP_LDA + e % n] = Sg[e];
    if (t < n) sM[t] = mu[t];
    sP[t] = 0.0, sMP[t] = 0.0, sLS[t] = 0.0;
    if (t == 0) snan = 0;
    __syncthreads();

    // ---- sweeps (_Sites.run / refine) ----
    int sweeps = 0;
    bool failed = false, numeric = false;
    for (int it = 0; it < 50; ++it) {
        ++sweeps;
        double total = 0.0;
        bool stop = false;
        for (int l = 0; l < n && !stop; ++l) {
            if (l == k) continue;
            const int idx = l < k ? l : l - 1;
            const double p = sP[idx], mp = sMP[idx];
            const double cVc = (sA[l * EP_LDA + l] - 2.0 * sA[k * EP_LDA + l] + sA[k * EP_LDA + k]) / 2.0;
            const double vc = t < n ? (sA[t * EP_LDA + l] - sA[t * EP_LDA + k]) / EP_SQRT2 : 0.0;
            const double cM = (sM[l] - sM[k]) / EP_SQRT2;
            const double cav_var = py_max(cVc / (1.0 - p * cVc), 0.0);
            const double cav_mean = cM + cav_var * (p * cM - mp);
            double z = cav_mean / sqrt(cav_var + 1e-25);
            if (isnan(z)) z = -__builtin_huge_val();
            if (z < -6.0) {             // factor certainly violated: minimiser k is dead
                failed = true;
                break;
            }
            double dp, dmp, d, p_out, mp_out, log_s;
            if (z > 6.0) {              // factor inactive: remove its message
                dp = -p, dmp = -mp;
                d = py_max(dmp, dp);
                p_out = 0.0, mp_out = 0.0, log_s = 0.0;
            } else {
                const double log_pdf = -0.5 * (z * z + EP_LOG_2PI);
                const double log_cdf = log(0.5 * erfc(-z / EP_SQRT2));
                const double ratio = exp(log_pdf - log_cdf);
                const double alpha = ratio / sqrt(cav_var);
                const double beta = alpha * (alpha * cav_var + cav_mean);
                const double r = beta / (1.0 - beta);
                const double p_new = r / cav_var;
                const double mp_new = r * (alpha + cav_mean / cav_var) + alpha;
                dp = py_max(-p + EP_EPS32, p_new - p);
                dmp = py_max(-mp + EP_EPS32, mp_new - mp);
                d = py_max(dmp, dp);
                p_out = p + dp, mp_out = mp + dmp;
                log_s = log_cdf - 0.5 * (log(beta) - log(p_out) - log(cav_var)) + (alpha * alpha) / (2.0 * beta) * cav_var;
            }
            const double denom = 1.0 + dp * cVc;
            const double coef = dp / denom;
            const double mcoef = (dmp - cM * dp) / denom;
            sVc[t] = vc;
            __syncthreads();            // every lane has read V's columns l, k and M before any row changes
            if (t < n) {
                bool bad = false;
                for (int j = 0; j < n; ++j) {
                    const double v = sA[t * EP_LDA + j] - coef * (vc * sVc[j]);
                    bad |= isnan(v);
                    sA[t * EP_LDA + j] = v;
                }
                sM[t] = sM[t] + mcoef * vc;
                if (bad) snan = 1;
            }
            if (t == 0) sP[idx] = p_out, sMP[idx] = mp_out, sLS[idx] = log_s;
            __syncthreads();
            if (snan) {                 // epmgp.py raises: "Resulting variance contains NaN"
                numeric = true;
                break;
            }
            if (isnan(d)) stop = true;  // run() returns (the sites stay as they are)
            else total += fabs(d);
        }
        if (failed || numeric || stop || fabs(total) < 0.001) break;
    }
    if (t == 0) sweeps_all[pk] = failed ? -1 : sweeps;
    if (numeric) {
        if (t == 0) kstat_all[pk] = ROBO_NUMERIC_ERROR;
        return;
    }
    double* dmu = with_deriv ? dmu_all + pk * nb : nullptr;
    double* dmumu = with_deriv ? dmumu_all + pk * nb * nb : nullptr;
    double* ds = with_deriv ? ds_all + pk * nt : nullptr;
    if (failed) {
        if (t == 0) logz_all[pk] = -__builtin_huge_val(), kstat_all[pk] = ROBO_OK;
        if (with_deriv) {
            for (int e = t; e < n; e += 64) dmu[e] = 0.0;
            for (int e = t; e < n * n; e += 64) dmumu[e] = 0.0;
            for (int e = t; e < nt; e += 64) ds[e] = 0.0;
        }
        return;
    }

    // ---- closed form (_log_normaliser) from the INPUT Sigma ----
    const int m = n - 1;
    const double c = 1.0 / EP_SQRT2, cn = -1.0 / EP_SQRT2;
    __syncthreads();
    for (int e = t; e < n * n; e += 64) sA[(e / n) * EP_LDA + e % n] = Sg[e];
    if (t < m) {
        const double sp = sqrt(sP[t]);
        sRv[t] = sp * c;                // R[l_a][a]
        sRk[t] = sp * cn;               // R[k][a]
    }
    // r = sum over the columns of shift * C: shift_a c in row l_a, sum_a shift_a (-c) in row k
    if (t < n) {
        double v;
        if (t == k) {
            v = 0.0;
            for (int a = 0; a < m; ++a) v = v + sMP[a] * cn;
        } else {
            v = sMP[t < k ? t : t - 1] * c;
        }
        sr[t] = v;
    }
    __syncthreads();
    // b = mu + Sigma r ; u = r^T Sigma (rSr = u . r)
    if (t < n) {
        double sr_ = 0.0, su_ = 0.0;
        for (int j = 0; j < n; ++j) sr_ = sr_ + sA[t * EP_LDA + j] * sr[j];
        for (int i = 0; i < n; ++i) su_ = su_ + sr[i] * sA[i * EP_LDA + t];
        sb[t] = mu[t] + sr_;
        su[t] = su_;
    }
    __syncthreads();
    // log det from the Cholesky of inner with the host's jitter ladder 0 / 1e-10 / 1e-6
    bool pd = false;
    const double ladder[3] = {0.0, 1e-10, 1e-6};
    for (int j = 0; j < 3 && !pd; ++j) {
        ep_build_inner(sA, sB, sRv, sRk, n, k, ladder[j]);
        pd = ep_cholesky(sB, sdiag, m);
        __syncthreads();
    }
    bool ok = pd;
    if (ok) {
        ep_build_inner(sA, sB, sRv, sRk, n, k, 0.0);
        ok = ep_lu(sB, spiv, m);
    }
    if (!ok) {
        if (t == 0) kstat_all[pk] = ROBO_NOT_POSITIVE_DEFINITE;
        return;
    }
    // G = inner^-1, column t in lane t (P e_t, unit-lower forward, upper backward), into sA (Sigma is no longer needed)
    __syncthreads();
    if (t < m) {
        for (int a = 0; a < m; ++a) sA[a * EP_LDA + t] = a == t ? 1.0 : 0.0;
        for (int a = 0; a < m; ++a) {
            const int p = spiv[a];
            if (p != a) {
                const double x = sA[a * EP_LDA + t];
                sA[a * EP_LDA + t] = sA[p * EP_LDA + t];
                sA[p * EP_LDA + t] = x;
            }
        }
        for (int a = 0; a < m; ++a) {
            double y = sA[a * EP_LDA + t];
            for (int b = 0; b < a; ++b) y = y - sB[a * EP_LDB + b] * sA[b * EP_LDA + t];
            sA[a * EP_LDA + t] = y;
        }
        for (int a = m - 1; a >= 0; --a) {
            double y = sA[a * EP_LDA + t];
            for (int b = a + 1; b < m; ++b) y = y - sB[a * EP_LDB + b] * sA[b * EP_LDA + t];
            sA[a * EP_LDA + t] = y / sB[a * EP_LDB + a];
        }
    }
    __syncthreads();
    // X = inner^-1 R^T: X[a][j] = G[a][a(j)] R_j (j != k), xk[a] = X[a][k] = sum_b G[a][b] R[k][b]
    if (t < m) {
        double v = 0.0;
        for (int b = 0; b < m; ++b) v = v + sA[t * EP_LDA + b] * sRk[b];
        sxk[t] = v;
    }
    __syncthreads();
    // A_raw = R X: row k (sum over a of R[k][a] X[a][j]) and column k (R_i xk[a(i)])
    if (t < n) {
        double v = 0.0;
        if (t == k) {
            for (int a = 0; a < m; ++a) v = v + sRk[a] * sxk[a];
        } else {
            const int at = t < k ? t : t - 1;
            for (int a = 0; a < m; ++a) v = v + sRk[a] * (sA[a * EP_LDA + at] * sRv[at]);
        }
        srowk[t] = v;
        scolk[t] = t == k ? v : sRv[t < k ? t : t - 1] * sxk[t < k ? t : t - 1];
    }
    __syncthreads();
    // A = (A_raw^T + A_raw) / 2, element by element
    auto a_raw = [&](int i, int j) -> double {
        if (i == k) return srowk[j];
        if (j == k) return scolk[i];
        const int ai = i < k ? i : i - 1, aj = j < k ? j : j - 1;
        return sRv[ai] * (sA[ai * EP_LDA + aj] * sRv[aj]);
    };
    auto a_sym = [&](int i, int j) -> double { return 0.5 * (a_raw(j, i) + a_raw(i, j)); };
    if (t < n) {
        double v = 0.0;
        for (int j = 0; j < n; ++j) v = v + a_sym(t, j) * sb[j];
        sAb[t] = v;
    }
    __syncthreads();
    if (t == 0) {
        double rSr = 0.0, bAb = 0.0, mur = 0.0, ls = 0.0, mpm = 0.0, logdet = 0.0;
        for (int j = 0; j < n; ++j) rSr = rSr + su[j] * sr[j];
        for (int j = 0; j < n; ++j) bAb = bAb + sb[j] * sAb[j];
        for (int j = 0; j < n; ++j) mur = mur + mu[j] * sr[j];
        for (int a = 0; a < m; ++a) ls = ls + sLS[a];
        for (int a = 0; a < m; ++a)
            if (sMP[a] != 0.0) mpm = mpm + sMP[a] * sMP[a] / sP[a];
        for (int a = 0; a < m; ++a) logdet = logdet + log(sdiag[a]);
        logdet = 2.0 * logdet;
        logz_all[pk] = 0.5 * (rSr - bAb - logdet) + mur + ls - 0.5 * mpm;
        kstat_all[pk] = ROBO_OK;
    }
    if (!with_deriv) return;
    // d_mu = r - Ab, d_mumu = -A, dS = -A - 2 r Ab^T + r r^T + (b^T A)^T Ab^T (b^T A = Ab: A is symmetric), symmetrised,
    // packed as the row-major lower triangle
    for (int e = t; e < n; e += 64) dmu[e] = sr[e] - sAb[e];
    for (int e = t; e < n * n; e += 64) {
        const int i = e / n, j = e - i * n;
        dmumu[e] = -a_sym(i, j);
    }
    auto ds_raw = [&](int i, int j) -> double {
        return -a_sym(i, j) - 2.0 * (sr[i] * sAb[j]) + sr[i] * sr[j] + sAb[i] * sAb[j];
    };
    for (int e = t; e < nt; e += 64) {
        int i = (int)((sqrt(8.0 * e + 1.0) - 1.0) / 2.0);
        while (i * (i + 1) / 2 > e) --i;
        while ((i + 1) * (i + 2) / 2 <= e) ++i;
        const int j = e - i * (i + 1) / 2;
        const double dij = ds_raw(i, j);
        ds[e] = 0.5 * (dij + ds_raw(j, i) - (i == j ? dij : 0.0));
    }
}

// grid: S workgroups of 256.  In place on the per-minimiser results of ep_site_kernel (joint_min's tail).
__global__ __launch_bounds__(256) void ep_epilogue_kernel(int nb, int with_deriv, double* __restrict__ logp_all,
                                                          double* __restrict__ dmu_all, double* __restrict__ dmumu_all,
                                                          double* __restrict__ ds_all, const int* __restrict__ kstat_all,
                                                          int* __restrict__ status_all) {
#pragma clang fp contract(off)
    __shared__ double sw[EP_MAX], szm[EP_MAX], sraw[EP_MAX];
    __shared__ int sbad;
    const int n = nb, t = threadIdx.x;
    const long long s = blockIdx.x;
    const int nt = n * (n + 1) / 2;
    double* logp = logp_all + s * nb;
    if (t == 0) {
        int st = ROBO_OK;
        for (int k = 0; k < n && st == ROBO_OK; ++k) st = kstat_all[s * nb + k];    // the host raises at the first k
        status_all[s] = st;
        sbad = st;
        if (st == ROBO_OK) {
            double* raw = sraw;
            double top = -__builtin_huge_val();
            for (int k = 0; k < n; ++k) {
                double v = logp[k];
                if (isinf(v)) v = -500.0;
                raw[k] = v;
                top = fmax(top, v);
            }
            double Z = 0.0, se = 0.0;
            for (int k = 0; k < n; ++k) Z = Z + exp(raw[k]);
            for (int k = 0; k < n; ++k) se = se + exp(raw[k] - top);
            double lse = top + log(se);
            if (isinf(lse)) lse = top;
            for (int k = 0; k < n; ++k) {
                logp[k] = raw[k] - lse;
                sw[k] = exp(raw[k]) / Z;
            }
        }
    }
    __syncthreads();
    if (sbad != ROBO_OK || !with_deriv) return;
    double* dmu = dmu_all + s * nb * nb;
    double* dmumu = dmumu_all + s * nb * nb * nb;
    double* ds = ds_all + s * nb * nt;
    if (t < n) {                     // Zm = p_min . dlogZ/dmu
        double v = 0.0;
        for (int k = 0; k < n; ++k) v = v + sw[k] * dmu[k * n + t];
        szm[t] = v;
    }
    __syncthreads();
    for (int e = t; e < n * n; e += 256) {   // gg = sum_k w_k (d_mumu_k + d_mu_k d_mu_k^T); d_mumu += -gg + Zm * Zm (sic)
        const int i = e / n, j = e - i * n;
        double g = 0.0;
        for (int k = 0; k < n; ++k) g = g + (dmumu[(size_t)k * n * n + e] + dmu[k * n + i] * dmu[k * n + j]) * sw[k];
        const double corr = -g + szm[j] * szm[j];
        for (int k = 0; k < n; ++k) dmumu[(size_t)k * n * n + e] = dmumu[(size_t)k * n * n + e] + corr;
    }
    for (int e = t; e < nt; e += 256) {       // Zs = p_min . dlogZ/dSigma
        double zs = 0.0;
        for (int k = 0; k < n; ++k) zs = zs + sw[k] * ds[(size_t)k * nt + e];
        for (int k = 0; k < n; ++k) ds[(size_t)k * nt + e] = ds[(size_t)k * nt + e] - zs;
    }
    __syncthreads();                          // every read of the raw d_mu is done
    for (int e = t; e < n * n; e += 256) dmu[e] = dmu[e] - szm[e % n];
}

// ---- device buffers: one grow-once set per context ----
struct EpWork {
    long long cap_s;    // beliefs the buffers hold at cap_nb
    int cap_nb;
    double *d_mu, *d_sigma, *d_logp, *d_dmu, *d_dmumu, *d_ds;
    int *d_sweeps, *d_kstat, *d_status;
};

void ep_release(robo_ctx* c) {
    EpWork* w = c->ep;
    if (!w) return;
    for (double* p : {w->d_mu, w->d_sigma, w->d_logp, w->d_dmu, w->d_dmumu, w->d_ds}) hipFree(p);
    for (int* p : {w->d_sweeps, w->d_kstat, w->d_status}) hipFree(p);
    delete w;
    c->ep = nullptr;
}

static int ep_ensure(robo_ctx* c, long long S, int nb) {
    if (c->ep && c->ep->cap_s >= S && c->ep->cap_nb >= nb) return ROBO_OK;
    const long long cs = c->ep ? (S > c->ep->cap_s ? S : c->ep->cap_s) : S;
    const int cnb = c->ep ? (nb > c->ep->cap_nb ? nb : c->ep->cap_nb) : nb;
    ROBO_HIP_CHECK(hipStreamSynchronize(c->stream));
    ep_release(c);
    EpWork* w = new EpWork();
    c->ep = w;
    const size_t n1 = (size_t)cs * cnb, n2 = n1 * cnb, n3 = n2 * cnb, nt = n1 * (cnb + 1) / 2 * cnb;
    ROBO_HIP_CHECK(hipMalloc((void**)&w->d_mu, n1 * sizeof(double)));
    ROBO_HIP_CHECK(hipMalloc((void**)&w->d_sigma, n2 * sizeof(double)));
    ROBO_HIP_CHECK(hipMalloc((void**)&w->d_logp, n1 * sizeof(double)));
    ROBO_HIP_CHECK(hipMalloc((void**)&w->d_dmu, n2 * sizeof(double)));
    ROBO_HIP_CHECK(hipMalloc((void**)&w->d_dmumu, n3 * sizeof(double)));
    ROBO_HIP_CHECK(hipMalloc((void**)&w->d_ds, nt * sizeof(double)));
    ROBO_HIP_CHECK(hipMalloc((void**)&w->d_sweeps, n1 * sizeof(int)));
    ROBO_HIP_CHECK(hipMalloc((void**)&w->d_kstat, n1 * sizeof(int)));
    ROBO_HIP_CHECK(hipMalloc((void**)&w->d_status, (size_t)cs * sizeof(int)));
    w->cap_s = cs, w->cap_nb = cnb;
    return ROBO_OK;
}

}  // namespace robo

using namespace robo;

extern "C" int32_t robo_ep_joint_min(robo_ctx* ctx, int32_t S, int32_t nb, const double* mu, const double* sigma,
                                     int32_t with_derivatives, double* logP, double* dlogPdMu, double* dlogPdSigma,
                                     double* dlogPdMudMu, int32_t* out_sweeps, int32_t* out_status) {
    if (!ctx || S < 1 || nb < 1 || nb > EP_MAX || !mu || !sigma || !logP || !out_status) return ROBO_BAD_ARGUMENT;
    if (with_derivatives && (!dlogPdMu || !dlogPdSigma || !dlogPdMudMu)) return ROBO_BAD_ARGUMENT;
    const int wd = with_derivatives ? 1 : 0;
    ROBO_HIP_CHECK(hipSetDevice(ctx->device));
    ROBO_TRY(ep_ensure(ctx, S, nb));
    EpWork* w = ctx->ep;
    hipStream_t st = ctx->stream;
    const size_t n1 = (size_t)S * nb, n2 = n1 * nb, n3 = n2 * nb, nt = n1 * (nb + 1) / 2 * nb;
    ROBO_HIP_CHECK(hipMemcpyAsync(w->d_mu, mu, n1 * sizeof(double), hipMemcpyHostToDevice, st));
    ROBO_HIP_CHECK(hipMemcpyAsync(w->d_sigma, sigma, n2 * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ep_site_kernel, dim3((unsigned)n1), dim3(64), 0, st, (int)nb, (const double*)w->d_mu,
                       (const double*)w->d_sigma, wd, w->d_logp, w->d_dmu, w->d_dmumu, w->d_ds, w->d_sweeps, w->d_kstat);
    ROBO_LAUNCH_CHECK();
    hipLaunchKernelGGL(ep_epilogue_kernel, dim3((unsigned)S), dim3(256), 0, st, (int)nb, wd, w->d_logp, w->d_dmu,
                       w->d_dmumu, w->d_ds, (const int*)w->d_kstat, w->d_status);
    ROBO_LAUNCH_CHECK();
    ROBO_HIP_CHECK(hipMemcpyAsync(logP, w->d_logp, n1 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (wd) {
        ROBO_HIP_CHECK(hipMemcpyAsync(dlogPdMu, w->d_dmu, n2 * sizeof(double), hipMemcpyDeviceToHost, st));
        ROBO_HIP_CHECK(hipMemcpyAsync(dlogPdSigma, w->d_ds, nt * sizeof(double), hipMemcpyDeviceToHost, st));
        ROBO_HIP_CHECK(hipMemcpyAsync(dlogPdMudMu, w->d_dmumu, n3 * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    if (out_sweeps) ROBO_HIP_CHECK(hipMemcpyAsync(out_sweeps, w->d_sweeps, n1 * sizeof(int), hipMemcpyDeviceToHost, st));
    ROBO_HIP_CHECK(hipMemcpyAsync(out_status, w->d_status, (size_t)S * sizeof(int), hipMemcpyDeviceToHost, st));
    ROBO_HIP_CHECK(hipStreamSynchronize(st));
    return ROBO_OK;
}
