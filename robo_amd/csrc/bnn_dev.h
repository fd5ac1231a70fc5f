// BOHAMIANN: a Bayesian neural network sampled by scale-adapted SGHMC on the device (bnn.hip, api_bnn.hip): the handle, what
// the host passes to the kernels and the owner layout of the sampler state.  The rule is stated in include/robo_hip.h.
//
// THE OWNER LAYOUT.  The chain kernel's gradient never leaves registers (MlpGrad, mlp_dev.h): every one of the P + 1 entries
// of a chain belongs to the thread that holds its gradient -- a dW entry to the lane and register of the matrix instruction's
// accumulator it is summed in, a bias to thread j, w_out[j] to thread 64 + j, b_out to thread 128, the log noise variance to
// thread 129.  A thread has BNN_SLOTS = 52 slots: q = ((l 2 + i) 2 + j) 4 + r for register r of accumulator (l, i, j), 48 + l
// for layer l's bias, 51 for the output layer and the noise.  The sampler state of slot q of thread t is element q WG + t of
// each of the chain's BNN_ARRAYS arrays [v | tau | gbar | V | M | sigma] of BNN_OWN doubles: the 64 lanes of a wave touch 64
// consecutive doubles per slot and array.  Slots that own nothing (pad rows and columns, tiles past the grid) are never read.
#pragma once
#include "blr_dev.h"

namespace robo {

constexpr int BNN_SLOTS = 52;
constexpr int BNN_OWN = BNN_SLOTS * WG;
constexpr int BNN_ARRAYS = 6;
constexpr int BNN_MAX_BATCH = ROBO_BNN_MAX_BATCH;          // four tiles of MLP_TR rows

struct BnnRun {                   // what one launch of the chain kernel is passed; every pointer device memory
    MlpNet net;
    int C, batch;
    long long n;
    const double *rows, *y;       // n x dim, n
    double* params;               // C x (P + 1): every chain's [p | l] at the launch's start and end
    double* state;                // C x BNN_ARRAYS x BNN_OWN (the owner layout)
    double* samples;              // ROBO_BNN_MAX_SAMPLES x (P + 1)
    int* status;                  // C x 2: [0] 0 fine, 1 a parameter left the finite numbers; [1] the call's steps before that
    const int* idx;               // the call's n_steps x batch row indices, or nullptr: drawn here
    const double* xi;             // the call's n_steps x C x (P + 1) normals, or nullptr: drawn here
    double* trace;                // the call's (n_steps + 1) x C x 5 x (P + 1), or nullptr
    long long call_t0, t0;        // the global step count at the call's and at this launch's start
    int steps, final;             // of this launch; it is the call's last (the trace's last row is written)
    long long burn, form_at;      // n_burn_in; the step in front of which M and sigma are formed from V (-1: they stand)
    int keep, s0;                 // keep_every; samples in the table at the call's start
    long long keeps0;             // kept steps among the step counts 1 .. call_t0
    double bd, eps2, eps4, c2, mdecay;      // |B|, eps^2, eps^4, 2 eps^2 mdecay
    double lam_n, inv_sn, ln_mu;  // lambda / n, 1 / (s_l n), ln mu_l
    unsigned long long seed;
};
// kept steps among the step counts 1 .. T
__host__ __device__ inline long long bnn_keeps(long long T, long long burn, int keep) { return T > burn ? (T - burn) / keep : 0; }

int launch_bnn_fill(robo_ctx* ctx, double* d_state, int C);
int launch_bnn_chain(robo_ctx* ctx, const BnnRun& a);
int launch_bnn_pack(robo_ctx* ctx, const MlpNet& net, const double* d_samples, int S, double* d_pads);
int launch_bnn_sweep(robo_ctx* ctx, const MlpNet& net, const double* d_pads, const double* d_samples, int S,
                     const double* d_rows, long long m, double y_mean, double y_std, int add_noise, double* d_mean,
                     double* d_var, double* d_per_sample);

}  // namespace robo

struct robo_bnn {
    robo_ctx* ctx;
    robo::MlpNet net;
    int C;
    bool has_state;
    long long steps;              // sampler steps taken since robo_bnn_set_state
    int n_samples;
    bool pads_stale;              // the padded copies do not show the sample table
    double y_mean, y_std;
    int add_noise;
    bool ms_valid;                // M and sigma in d_state were formed with (ms_eps2, ms_mdecay)
    double ms_eps2, ms_mdecay;
    double *d_params, *d_state, *d_samples;
    int* d_status;
    double* d_pads;               // n_samples x mlp_pad_len (grows)
    size_t pads_cap;
    double* d_rows;               // a run's [X (n x dim) | y (n)] (grows)
    size_t rows_cap;
    int* d_idx;                   // a run's indices (grows)
    size_t idx_cap;
    double* d_xi;                 // a run's normals (grows)
    size_t xi_cap;
    double* d_trace;              // (grows)
    size_t trace_cap;
    double* d_cand;               // the uploaded candidate rows (grows)
    size_t cand_cap;
    double* d_ps;                 // per-sample values (S x m) of a call that asks (grows)
    size_t ps_cap;
    robo_cand* k;                 // the moments' tables and the acquisition's state, kept between calls of one m
};
