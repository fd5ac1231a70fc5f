/*
 * robo_hip.h -- C ABI of librobo_hip.so: the MI355X (gfx950) GP-posterior + acquisition
 * hot path of automl/RoBO.
 *
 * This is the drop-in boundary.  The reference has no native
 * code; the arithmetic it delegates to the george C++ library through the call sites
 * listed below is what these entry points replace.  A RoBO maintainer binds them with
 * ctypes; robo_amd/_lib.py is exactly that binding.
 *
 * Conventions
 *   - every function returns a robo_status (int32); 0 = OK
 *   - all matrices are row-major (C order) IEEE fp64, exactly what NumPy hands over
 *   - "host" pointers are caller-owned and only read/written during the call
 *   - handles own all device memory; nothing is allocated per call on the hot path
 *   - a handle is not thread-safe; one HIP stream per context; no callbacks
 *   - theta is the reference's log-space hyper-parameter vector
 *       [log amp, log m_1 .. log m_D, log sigma^2]           (P = D + 2; ROBO_KERNEL_FABOLAS: see enum)
 *     (robo/models/gaussian_process.py:110-114,151-152; robo/priors/default_priors.py:28-35)
 */
#ifndef ROBO_HIP_H
#define ROBO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct robo_ctx robo_ctx;   /* one device + one HIP stream + event slots            */
typedef struct robo_gp robo_gp;     /* one GP: training data, Cholesky factor, solve vector */
typedef struct robo_cand robo_cand; /* one device-resident candidate batch + its workspace  */

enum robo_status {
    ROBO_OK = 0,
    ROBO_NOT_POSITIVE_DEFINITE = 1, /* -> np.linalg.LinAlgError (gaussian_process.py:120,156;
                                          gaussian_process_mcmc.py:194-197)                  */
    ROBO_NOT_FITTED = 2,            /* -> Exception('Model has to be trained first!')
                                          (gaussian_process.py:241,273,322)                  */
    ROBO_BAD_SHAPE = 3,             /* the reference asserts (base_model.py:68-70,76)        */
    ROBO_RUNTIME_ERROR = 4,         /* HIP error; text in robo_last_error_string()           */
    ROBO_BAD_ARGUMENT = 5,
    ROBO_NUMERIC_ERROR = 6          /* -> Exception('... Resulting variance contains NaN')
                                          (robo/util/epmgp.py: the EP working covariance)   */
};

enum robo_kernel_kind {
    ROBO_KERNEL_MATERN52_ARD = 0, /* amp * george.kernels.Matern52Kernel(metric, ndim=D)
                                     (robo/fmin/bayesian_optimization.py:75-81)              */
    ROBO_KERNEL_RBF_ARD = 1,      /* amp * george.kernels.ExpSquaredKernel(metric, ndim=D)   */
    ROBO_KERNEL_FABOLAS = 2       /* amp * prod_d Matern52Kernel(m_d, axes=d) * BayesianLinearRegressionKernel(
                                     log_a, log_b, axes=D)   (robo/fmin/fabolas.py:104-117).  dim = D + 1: the
                                     last input column is the basis-transformed fidelity u (fabolas_gp.py:122-126);
                                     theta = [log amp, log m_1..m_D, log_a, log_b, log sigma^2]  (P = dim + 3)    */
};

enum robo_acq_kind {
    ROBO_ACQ_EI = 0,     /* robo/acquisition_functions/ei.py:65-88      */
    ROBO_ACQ_LOG_EI = 1, /* robo/acquisition_functions/log_ei.py:74-120 */
    ROBO_ACQ_PI = 2,     /* robo/acquisition_functions/pi.py:57-63      */
    ROBO_ACQ_LCB = 3     /* robo/acquisition_functions/lcb.py:62-65     */
};

/* flags reported by the acquisition kernels (host shim applies the reference's guards) */
#define ROBO_FLAG_ZERO_SIGMA 1u   /* some s == 0           (ei.py:72-74)  */
#define ROBO_FLAG_NEGATIVE_EI 2u  /* some EI < 0           (ei.py:86-88)  */
#define ROBO_FLAG_NAN 4u          /* some acquisition value is NaN        */
#define ROBO_FLAG_NOT_FACTORED 8u /* Monte-Carlo information gain: some candidate's covariance
                                     had no Cholesky factor with jitter up to 1e4              */
#define ROBO_FLAG_FROZEN 16u      /* gradient refinement: some start stopped early (variance on its floor, value
                                     not finite, or no ascent direction left inside the box)   */

/* ---- context ---------------------------------------------------------------------- */
int32_t robo_device_count(int32_t* out_n);
/* hip_stream: an existing hipStream_t to launch on (e.g. torch's current stream), or NULL
 * to let the library create its own non-blocking stream.                                  */
int32_t robo_ctx_create(int32_t device, void* hip_stream, robo_ctx** out);
/* Handles created on a context (robo_gp, robo_cand, robo_comm, robo_multi) keep it alive: robo_ctx_destroy on a context
 * that still has such handles only marks it; its stream, events and scratch are released with the last of them.  (A
 * garbage-collected binding cannot promise to finalise a context after everything that lives on it.)                     */
int32_t robo_ctx_destroy(robo_ctx* ctx);
/* contexts whose resources are still held (created and not yet released): diagnostics / tests                            */
int32_t robo_ctx_live_count(int32_t* out_n);
int32_t robo_ctx_synchronize(robo_ctx* ctx);
int32_t robo_ctx_device_name(robo_ctx* ctx, char* buf, int32_t buf_len);
/* HIP-event timing on the context's stream (what bench.py uses).  There are 34 slots, 0 .. 33.  Slots 0 .. 18 are the
 * caller's; the library records the others itself (csrc/common.h names them; a pair is shared by calls that never run
 * inside one another):
 *   19 .. 23  the phases of robo_gp_fit: 19 -> 21 gram kernel, 20 -> 21 gram phase, 21 -> 22 Cholesky, 22 -> 23
 *             log-likelihood.  Only when switched on with robo_ctx_set_phase_events (off by default: four event packets
 *             cost a 1.8 ms fit ~30 us; the environment variable ROBO_PHASE_EVENTS=1 switches them on at context creation).
 *   24 .. 27  the phases of the posterior evaluation of the last candidate chunk: 24 -> 25 cross-gram, 25 -> 26 triangular
 *             solve, 26 -> 27 post.  "The condition of slots 24..27", which the pairs below share unless they say
 *             otherwise: recorded for every batch above 16 384 rows, for smaller ones only when the phase events are
 *             switched on.
 *   28, 29    robo_gp_grad_loglik: everything after the factorisation (always recorded); the descent launch of
 *             robo_paths_descend (always) and of robo_paths_refine_cand.
 *   30, 31    what follows the sweeps: the envelope kernel of robo_kg_eval_cand and the element-wise half of
 *             robo_mes_eval_cand (last sample each), the strip kernel of robo_ehvi_eval_cand, the passes of the path kernel
 *             (robo_paths_eval_cand, robo_paths_refine_cand), the fold kernel of robo_qei_batch_cand's last pick.
 *   32, 33    the fold kernel of robo_cei_eval_cand.                                                                    */
int32_t robo_ctx_event_record(robo_ctx* ctx, int32_t slot);
int32_t robo_ctx_event_elapsed_ms(robo_ctx* ctx, int32_t slot_begin, int32_t slot_end, float* out_ms);
int32_t robo_ctx_set_phase_events(robo_ctx* ctx, int32_t on);
/* Tuning knobs of a context.  They are read from the environment ONCE, when the context is created (variable
 * ROBO_<KEY in upper case>), and changed afterwards only through this call; value INT64_MIN restores the default, key
 * "env" re-reads all variables.  Keys: ws_bytes (solve workspace per candidate handle, default 6 GiB),
 * winv_max / winv_min_blocks (batches of at most winv_max candidates on a factor of at least winv_min_blocks 128-row
 * blocks are evaluated through the explicit inverse factor, winv.hip; default 32768 / 6, measured r03b; 0 = never),
 * winv_cond_max (... while cond_inf(L) <= this, default 1e5: robo_gp_factor_cond), winv_rows (form of that product: -1 auto,
 * 0 chunked units + reduction pass, 1 one workgroup per (candidate tile, block row) over the whole contraction range),
 * trsm_pair (1: two block rows of the solve per launch on one read of V; default 0: one), trsm_small_max, trsm_small_narrow,
 * trsm_small_deep, trsm_rows, predict_stepwise, mcmc_block_step (the chain's one-launch half-step of one-block problems:
 * 0 never, 1 up to 63 points, 2 = default: all of them; a larger value means 2), potrf_fused, potrf_tm4_min,
 * potrf_max_wg, potrf_group, potrf_split (sub-batches of a batched factorisation on their own streams, default 3, from
 * potrf_split_min = 12 panels on), potrf_lead, potrf_thin_last (kernel-variant selection; A/B runs and tests),
 * acq_screen (1 = default: an argmax-only acquisition call skips the candidates that cannot win, see robo_acq_eval_cand;
 * 0 never), acq_screen_min (batches above this many candidates are screened; -1 = default: winv_max, the size above which
 * the unscreened call is the block-row substitution; tests lower it), acq_screen_keep_max (percent of the batch that may
 * survive the screen, default 25: more than that and the call falls back to the plain sweep), acq_screen_dot (which kernel
 * forms the screen's bounds: -1 = default: the dot-form kernel, whose squared distances come from the fp64 matrix
 * instruction on centred coordinates, for Matern-5/2 and RBF up to D = 32 where the fitted theta's worst-case distance
 * error stays within 1e-12, the direct-difference kernel otherwise; 0 never the dot form; 1 wherever the kind and D permit,
 * whatever the error: tests.  Both give rigorous bounds, so results do not depend on it), acq_screen_lean (how the dot-form
 * kernel finishes a pair: -1 = default: the lean finish, which evaluates the covariance to a proven 8e-13 amp and adds 1e4
 * times that error to the margin, where that term stays within 1e-2 of the prior standard deviation, the finish to the
 * last bit otherwise; 0 never the lean finish; 1 wherever the dot-form kernel runs: tests.  Rigorous bounds either way),
 * acq_screen_single (a single-precision first stage in front of that pass: -1 = default: where the lean finish is selected
 * and the first stage's own margin, 1.5 times a proven 6.3e-7 amp per covariance, stays within half the prior standard
 * deviation, an argmax-only call first forms its bounds with a single-precision finish and solves that stage's survivors
 * when they fit one tile of 128 and the cap; otherwise the fp64 pass runs as before and the factor's first stage pauses for
 * 1, 2, 4, ... calls; 0 never; 1 wherever the lean finish runs; 2 as 1, and robo_acq_screen_bounds returns the first
 * stage's bounds: tests.  Rigorous bounds either way, same results),
 * acq_screen_int (how that first stage forms its squared distances: -1 = default: for 8 < D <= 16, from exact int8 matrix
 * products of the centred coordinates on a 24-bit grid spanning twice the training rows' extent, where the rows have an
 * extent and the stage's margin with the grid's proven error added still stays within half the prior standard deviation,
 * from the fp64 matrix instruction otherwise; 0 never the integer form; 1 wherever the first stage runs and D <= 16: tests.
 * Rigorous bounds either way, same results),
 * acq_screen_fused_tail (1 = default: when the screen's survivors fit one block of 256, their output transform, acquisition
 * values, argmax, index map and report run as one single-workgroup launch; 0: the five launches.  Same bits either way),
 * trsm_chain (small batches on two or more block rows, solved by ONE launch whose block rows hand their tiles to each
 * other instead of one launch per block row, trsm_chain.hip: -1 = default: automatic (from three block rows on, while the
 * launch stays within trsm_chain_max_wg), 0 never, 1 wherever legal (from two block rows on); taken by
 * robo_gp_predict[_cand], robo_gp_predict_cov, robo_acq_eval[_cand] and robo_acq_eval_marginal_cand, bit-identical
 * results; a launch whose hand-off times out is repeated by launches, the context stays off the chain until this key is
 * set again, and robo_last_error_string says so although the call succeeds), trsm_chain_max_wg (the automatic rule:
 * while 16-candidate tiles x block rows <= this many times the CU count), trsm_chain_spin_limit (tests only).           */
int32_t robo_ctx_set_tuning(robo_ctx* ctx, const char* key, int64_t value);
const char* robo_last_error_string(void);
const char* robo_version_string(void);

/* ---- GP fit: replaces george.GP.compute + log_likelihood ---------------------------
 * call sites: robo/models/gaussian_process.py:119,122,155,159,173;
 *             robo/models/gaussian_process_mcmc.py:195,200-202                          */
int32_t robo_gp_create(robo_ctx* ctx, int32_t kernel_kind, int32_t n_max, int32_t dim, robo_gp** out);
int32_t robo_gp_destroy(robo_gp* gp);
/* X: (n, dim) inputs as the GP sees them (already [0,1]-normalised by the caller,
 * gaussian_process.py:91); y: (n,) targets.  Uploaded once; thousands of theta are then
 * evaluated on the same data (the MCMC / L-BFGS loops).                                   */
int32_t robo_gp_set_data(robo_gp* gp, const double* X, const double* y, int32_t n);
/* un-normalisation applied to predictions: mu*y_std + y_mean, var*y_std^2
 * (gaussian_process.py:282-284).  Default (0, 1).                                          */
int32_t robo_gp_set_output_transform(robo_gp* gp, double y_mean, double y_std);
/* 0 (default): covariance entries in fp64.  1: evaluated in fp32 and widened -- the mixed
 * precision "fp32 K-build + fp64 Cholesky" of BASELINE.json config 5 (applies to K and K*).  */
int32_t robo_gp_set_precision(robo_gp* gp, int32_t fp32_gram);
/* number of theta entries for a kernel kind and input dimension                              */
int32_t robo_theta_size(int32_t kernel_kind, int32_t dim);
/* K = k_theta(X,X) + (sigma^2 + 1.25e-12) I ; L = chol(K) ; z = L^-1 (y - mean_c);
 * loglik = -1/2 (z.z + 2 sum log L_ii + n log 2pi).  On ROBO_NOT_POSITIVE_DEFINITE
 * *out_fail_col is the 0-based failing column and the GP is left unfitted.
 * out_loglik / out_fail_col may be NULL.                                                   */
int32_t robo_gp_fit(robo_gp* gp, const double* theta, double mean_c, double* out_loglik, int32_t* out_fail_col);
/* Analytic gradient of the log marginal likelihood w.r.t. theta (log-space), fitted at theta on
 * return like robo_gp_fit.  Replaces the body of GaussianProcess.grad_nll
 * (robo/models/gaussian_process.py:168-191: K^-1 via solver.apply_inverse, kernel.gradient (N,N,P),
 * 0.5 einsum('ijk,ij', Kg, alpha alpha^T - K^-1)) without forming K^-1 or the gradient tensor on
 * the host.  out_grad[theta_size]: d loglik / d theta_p for the kernel parameters; the LAST entry is
 * 0.5 tr(alpha alpha^T - K^-1) = d loglik / d sigma^2 (not d / d log sigma^2) exactly as the
 * reference computes it (:178-182 use the identity as the noise "gradient").  Prior gradients and
 * the sign flip of grad_nll stay with the caller.                                               */
int32_t robo_gp_grad_loglik(robo_gp* gp, const double* theta, double mean_c, double* out_loglik,
                            double* out_grad, int32_t* out_fail_col);

/* S independent likelihood evaluations on the same data in ONE batched pass (every kernel of
 * the fit runs with S x the workgroups); out_status[s] is a robo_status.  Works on a separate
 * batch workspace; the GP itself is left UNFITTED (call robo_gp_fit for the theta to keep).    */
int32_t robo_gp_loglik_batch(robo_gp* gp, const double* thetas, int32_t S, double mean_c, double* out_loglik,
                             int32_t* out_status);

/* S likelihoods AND gradients in ONE batched pass per workspace group: per sample exactly robo_gp_grad_loglik's result, bit
 * for bit (out_grad is S x theta_size, the last entry of a row d / d sigma^2 as there), on the batch workspace of
 * robo_gp_loglik_batch plus two n_pad x n_pad matrices per sample; samples go in groups that fit the context's ws_bytes
 * (ROBO_BAD_SHAPE if not even one does), one synchronisation per group.  out_status[s] (nullable) is a robo_status: a
 * non-finite theta gives ROBO_BAD_ARGUMENT, a failed factorisation ROBO_NOT_POSITIVE_DEFINITE -- log-likelihood -inf and a
 * NaN gradient for that sample only.  The GP itself is left UNFITTED.                                                        */
int32_t robo_gp_grad_loglik_batch(robo_gp* gp, const double* thetas, int32_t S, double mean_c, double* out_loglik,
                                  double* out_grad, int32_t* out_status);

/* Multi-start MAP optimisation of the hyper-parameters, resident on the device: replaces the host loop of
 * GaussianProcess.optimize (robo/models/gaussian_process.py:193-219, SciPy's L-BFGS-B on finite differences of nll from one
 * start).  Maximises F(theta) = log p(y | X, theta) + log prior(theta) with prior_kind / prior_par exactly those of
 * robo_gp_mcmc_run; F is invalid (the reference's protocol) when any |theta_p| > 20, the factorisation fails or the prior
 * is +-inf or NaN.  Its gradient G is robo_gp_grad_loglik's with the last entry times exp(theta_last) (the chain rule
 * to log sigma^2) plus the analytic gradient of the prior.
 * All n_starts (1 .. 64) starts (n_starts x P) run in lock step, one batched evaluation of (F, G) per iteration, no read-back
 * in between.  Iteration 0 evaluates the starts clipped to the box [lower, upper] (P each): an invalid F makes a start dead,
 * otherwise alpha := step0.  Iteration t >= 1, per live start (x, f, g): d = the L-BFGS two-loop direction of its last
 * <= history (1 .. 16) pairs (s_i, y_i), scaled by s.y / y.y of the newest (no pairs: g / |g|); d_p := 0 where x_p sits on a
 * bound and d_p points out; if d.g <= 0 the pairs are dropped and d = the projected g, normalised (zero: the start freezes,
 * "no direction"); trial z = clip(x + alpha d).  Accepted iff F(z) is valid and F(z) >= f + c1 (z - x).g: then the pair
 * (z - x, g - G(z)) is pushed if s.y > 1e-10 |s| |y| (the oldest drops), x := z, alpha := 1, and the start freezes as
 * "converged" if the largest projected |G_p| <= gtol.  Rejected: alpha := alpha / 2, below 2^-40 the start freezes,
 * "stalled".  The start with the largest final F wins (ties: the first; dead starts never): out_theta (P), *out_value,
 * *out_best -- -1 and NaN if every start is dead, which is not an error.  Per start, nullable: out_final (n_starts x P),
 * out_values, out_status (0 ran out of iterations, 1 converged, 2 stalled or no direction, 3 dead).
 * out_trace (nullable): (n_iters + 1) x n_starts x (2 P + 3) = [trial theta | F | G | the alpha it was made with | code],
 * code 1 accepted, 0 rejected, 2 frozen earlier (the entry repeats the start's point), 3 trial invalid (F -inf, G NaN).
 * Fixed summation orders: two calls return the same bits.  ROBO_BAD_SHAPE if the starts do not fit the workspace
 * (ws_bytes) in one pass.  One synchronisation; state is kept with gp between calls of one (n_starts, P); leaves the GP
 * unfitted.                                                                                                                  */
int32_t robo_gp_optimize_hypers(robo_gp* gp, double mean_c, int32_t prior_kind, const double* prior_par,
                                const double* lower, const double* upper, const double* starts, int32_t n_starts,
                                int32_t n_iters, int32_t history, double step0, double c1, double gtol,
                                double* out_theta, double* out_value, int32_t* out_best, double* out_final,
                                double* out_values, int32_t* out_status, double* out_trace);

/* The hyper-parameter chain of GaussianProcessMCMC.train, resident on the device: replaces
 *     sampler = emcee.EnsembleSampler(n_hypers, ndim, self.loglikelihood); sampler.run_mcmc(p0, n_steps, rstate0=rng)
 * (robo/models/gaussian_process_mcmc.py:114-142) INCLUDING emcee 2's stretch move, the prior and the accept test -- one
 * sequence of launches, no host round trip between half-steps.  lnprob(theta) = log p(y | X, theta) + log prior(theta)
 * with the reference's protocol (:185-202: any |theta_p| > 20, or a factorisation that fails -> -inf).
 * prior_kind 0 = none, 1 = robo.priors.default_priors.DefaultPrior with prior_par = {lognormal loc, lognormal sigma,
 * tophat min, tophat max, horseshoe scale}, 2 = robo.priors.env_priors.EnvPrior (robo/priors/env_priors.py:8-54, the prior
 * robo/fmin/fabolas.py:120-127 gives FabolasGPMCMC, robo/models/fabolas_gp.py:49-77) with prior_par = {those five, n_ls,
 * n_lr, normal mean, normal sigma}: tophat on theta[1 .. n_ls] only, plus NormalPrior.lnprob -- a pdf, as in the
 * reference (robo/priors/base_prior.py:357) -- of each of the n_lr regression parameters behind them.  The random numbers of a stretch-move chain do not depend on its state: the
 * caller draws them in emcee 2's order -- per step and half-ensemble rand(k/2) for z, randint(k/2) for the partners,
 * rand(k/2) for the accept test -- into u_stretch / partner / u_accept, each [n_steps][2][k/2].
 * pos (k x P) and lnp (k): in = start positions (lnp evaluated here when eval_start != 0), out = final state;
 * out_chain (k x n_steps x P), out_lnprob (k x n_steps), out_accepted (k) nullable.  a = 2 in emcee.
 * ROBO_BAD_ARGUMENT with emcee's message if a log-probability is NaN or the initial one +inf.  Leaves the GP unfitted. */
int32_t robo_gp_mcmc_run(robo_gp* gp, double mean_c, int32_t prior_kind, const double* prior_par, int32_t n_walkers,
                         int32_t n_steps, double a, const double* u_stretch, const int32_t* partner,
                         const double* u_accept, int32_t eval_start, double* pos, double* lnp, double* out_chain,
                         double* out_lnprob, int64_t* out_accepted);
/* Host helper of robo_gp_mcmc_run: the random numbers of n_steps ensemble steps exactly as a legacy
 * numpy.random.RandomState produces them in emcee 2's order -- per half-step rand(half), randint(half, size=half),
 * rand(half) -- from the MT19937 state (key[624], pos) of RandomState.get_state(), which is advanced in place (hand it back
 * with set_state).  Outputs [n_steps][2][half].  Pure host code; replaces 6 n_steps NumPy calls.                     */
int32_t robo_mcmc_draws(uint32_t* mt_key, int32_t* mt_pos, int32_t n_steps, int32_t half, double* u_stretch,
                        int32_t* partner, double* u_accept);
/* The per-sample model fits of GaussianProcessMCMC.train (gaussian_process_mcmc.py:149-164: one
 * GaussianProcess per hyper-parameter sample, each a gp.compute on the SAME X, y) as one batched pass
 * that KEEPS the factors: gps[0] holds the training data (robo_gp_set_data); afterwards every gps[s]
 * with out_status[s] == ROBO_OK is a fitted handle at thetas[s] (own copy of the data, factor, diagonal
 * block inverses, scaled inputs), bit-identical to robo_gp_fit(gps[s], thetas[s]).  Samples whose K is not
 * positive definite are left unfitted with out_status[s] = ROBO_NOT_POSITIVE_DEFINITE (the caller applies
 * the reference's noise x 10 retry, gaussian_process.py:120-122, to those).  All handles: same context,
 * kernel kind, dim, n_max >= n, pairwise distinct.                                                   */
int32_t robo_gp_fit_batch(robo_gp* const* gps, int32_t S, const double* thetas, double mean_c, double* out_loglik,
                          int32_t* out_status);
/* copy the lower Cholesky factor (n x n, row-major, upper zeroed) back -- diagnostics/tests */
int32_t robo_gp_get_factor(robo_gp* gp, double* out_L);
int32_t robo_gp_get_gram(robo_gp* gp, const double* theta, double* out_K); /* K incl. noise, n x n  */
/* cond_inf(L) = |L|_inf |L^-1|_inf of the current factor, EXACT (row sums of L and of the explicit inverse W, which is
 * built for this factor if it has not been yet: ~1 ms at N = 4096, then cached until the next fit).  It is the number
 * that decides whether small candidate batches of robo_gp_predict* / robo_acq_eval* (the reference's
 * gp.predict, robo/models/gaussian_process.py:280-294) may go through W (forward error ~eps cond) or stay on the
 * block-row substitution: the explicit inverse is used while it is <= the context's `winv_cond_max` (default 1e5).
 * out[0] = cond_inf(L), out[1] = min L_ii, out[2] = max L_ii.  Diagnostics / tests.                         */
int32_t robo_gp_factor_cond(robo_gp* gp, double* out);
/* Start building that explicit inverse NOW, asynchronously (returns without waiting for the device): called right after the
 * final fit of GaussianProcess.train (robo/models/gaussian_process.py:119) so that the build (0.9 ms at N = 4096) runs while
 * the host prepares the next acquisition maximisation (robo/maximizers/random_sampling.py:38-47 draws its 500 candidates in
 * a Python loop) and the first robo_gp_predict* / robo_acq_eval* of a small batch finds W in place.  A no-op where a small
 * batch would not use W (factor of fewer than winv_min_blocks blocks, fp32 K-build, diagonal ratio beyond the bound) and
 * on a handle that has never evaluated a small batch through W (nothing is allocated or built speculatively for models
 * that only see large batches): from the second iteration of a loop on.                                            */
int32_t robo_gp_prefetch_inverse(robo_gp* gp);

/* ---- candidates --------------------------------------------------------------------- */
/* Xc: (m, dim) candidates in the GP's (normalised) input space; copied H2D here, once.    */
int32_t robo_cand_create(robo_ctx* ctx, const double* Xc, int64_t m, int32_t dim, robo_cand** out);
int32_t robo_cand_destroy(robo_cand* cand);
/* a new batch of the SAME size into an existing handle (H2D only; buffers and solve workspace are kept): what a BO
 * loop does once per iteration with robo/maximizers/random_sampling.py:38-47's fresh candidate matrix            */
int32_t robo_cand_set_points(robo_cand* cand, const double* Xc, int64_t m);
/* device-side generation, no H2D: uniform [0,1)^dim, counter-based (Philox-4x32-10)         */
int32_t robo_cand_create_uniform(robo_ctx* ctx, int64_t m, int32_t dim, uint64_t seed, robo_cand** out);
/* RandomSampling.maximize's candidate recipe on the device (random_sampling.py:38-47), in the
 * normalised space: rows < n_uniform uniform, the rest N(loc, scale) clipped to [0,1]
 * (loc = normalised incumbent, scale_d = 0.1 / (upper_d - lower_d)).                           */
int32_t robo_cand_create_random(robo_ctx* ctx, int64_t m, int32_t dim, uint64_t seed, int64_t n_uniform,
                                const double* loc, const double* scale, robo_cand** out);
/* points first_index .. first_index + m - 1 of a (scrambled) Sobol' sequence in [0,1)^dim, generated on the device
 * from the direction numbers sv (dim x bits, row-major) and the digital shift (dim):
 *   x_k[d] = (shift[d] ^ XOR_{b in gray(k)} sv[d][b]) / 2^bits.   BASELINE config 5 names 2^20 Sobol candidates
 * (scipy.stats.qmc.Sobol(d=64, scramble=True, seed=0).random_base2(20); the reference itself has no
 * Sobol sampler); with sv / shift of a SciPy engine the sequence equals engine.random() bit for bit, and a rank of a
 * candidate shard generates its own slice through first_index.                                            */
int32_t robo_cand_create_sobol(robo_ctx* ctx, int64_t m, int32_t dim, const uint64_t* sv, const uint64_t* shift,
                               int32_t bits, uint64_t first_index, robo_cand** out);
int32_t robo_cand_get_points(robo_cand* cand, double* out_Xc);
/* candidates per pass of the solve workspace of the LAST posterior evaluated on this handle (a multiple of 128; the
 * whole padded batch when it fits ROBO_WS_BYTES, default 6 GiB); 0 before the first evaluation.  Diagnostics: lets a
 * caller (tests) see that a batch was evaluated in several passes.                                              */
int32_t robo_cand_workspace_chunk(robo_cand* cand, int64_t* out_chunk);
/* name of the kernel that ran the solve of the last posterior on this handle ("" before the first): the library picks
 * it from the batch size and precision; bench.py labels its roofline block with it.  Diagnostics.  Where buf has room
 * behind that string's terminator a second string follows it: the kernel that formed the bounds of the last acquisition
 * screen on this handle ("screen_bounds_kernel", "screen_bounds_dot_kernel", "" before the first).                 */
int32_t robo_cand_last_solve_kernel(robo_cand* cand, char* buf, int32_t buf_len);
int32_t robo_cand_get_point(robo_cand* cand, int64_t index, double* out_x); /* one row: the winner */

/* ---- posterior: replaces george.GP.predict (gaussian_process.py:280-294) ------------ */
/* mean (m,), var (m,): diagonal only; var floored at DBL_EPSILON after the output
 * transform, exactly gaussian_process.py:282-294.  Either output may be NULL.
 * The host-array forms (robo_gp_predict, robo_acq_eval) keep the candidate handle they build inside the
 * robo_gp between calls of one batch size <= 16384 (the reference's 500 candidates per iteration, the 1 x D
 * calls of its single-point maximisers): a repeated call only re-uploads the points.                       */
int32_t robo_gp_predict_cand(robo_gp* gp, robo_cand* cand, double* out_mean, double* out_var);
int32_t robo_gp_predict(robo_gp* gp, const double* Xc, int64_t m, double* out_mean, double* out_var);
/* GaussianProcessMCMC.predict (gaussian_process_mcmc.py:205-249): mixture over S fitted GPs,
 * m = mean_s mu_s, v = var_s(mu_s) + mean_s(var_s), floored at DBL_EPSILON; NumPy's operation
 * order along the sample axis.                                                                */
int32_t robo_gp_predict_mixture_cand(robo_gp* const* gps, int32_t S, robo_cand* cand, double* out_mean,
                                     double* out_var);
/* full covariance (m x m), small m only (predict(full_cov=True), predict_variance,
 * sample_functions: gaussian_process.py:221-248,298-332)                                    */
/* Gradients of the posterior w.r.t. the test inputs: what model.predictive_gradients(X) supplies to the
 * reference's acquisition derivatives (robo/acquisition_functions/ei.py:80-85, pi.py:65-71, lcb.py:66-68) and to
 * robo/util/posterior_optimization.py:38-40,96-104 (no model in the reference tree implements it).
 * Xc (m x D) in the GP's normalised input space; out_dmean / out_dvar (m x D, row-major): derivatives of the
 * values out_mean / out_var w.r.t. those coordinates (output transform applied; the variance floor is not
 * differentiated).  Cost: D + 1 right-hand sides of the blocked forward substitution per point.            */
int32_t robo_gp_predict_grad(robo_gp* gp, const double* Xc, int64_t m, double* out_mean, double* out_var,
                             double* out_dmean, double* out_dvar);
int32_t robo_gp_predict_cov(robo_gp* gp, const double* Xc, int64_t m, double* out_mean, double* out_cov);

/* ---- acquisition: replaces EI/LogEI/PI/LCB.compute + the argmax of
 * RandomSampling.maximize (robo/maximizers/random_sampling.py:48-50) ------------------ */
/* out_acq (m,) may be NULL when only the maximiser is wanted.  argmax follows np.argmax:
 * first index of the maximum, NaN counts as maximal.  par = xi (EI/LogEI/PI) or kappa (LCB);
 * eta = incumbent value (ignored by LCB).
 * Argmax-only calls (out_acq == NULL, also of the sharded and multi-device forms) on a large batch are SCREENED: one
 * O(N) pass per candidate gives the posterior mean through alpha = L^-T z and, with the prior variance and the variance
 * floor, an upper and a lower bound of the acquisition value; only candidates whose upper bound reaches the best lower
 * bound are solved, by the block-row substitution the unscreened call runs, so (max, argmax, flags) are the unscreened
 * call's bit for bit.  Screened: EI, LogEI, PI, LCB with kappa >= 0, finite eta / par, one fitted GP with fp64
 * covariance entries, batches above `acq_screen_min`, max L_ii / min L_ii <= 1e4.  When more than `acq_screen_keep_max`
 * percent survive, the call runs the plain sweep and the factor is not screened again for 1, 2, 4, ... calls (until the
 * next fit).  After a screened call the handle holds no posterior of the whole batch.                               */
int32_t robo_acq_eval_cand(robo_gp* gp, int32_t acq_kind, double par, double eta, robo_cand* cand, double* out_acq,
                           double* out_max, int64_t* out_argmax, uint32_t* out_flags);
int32_t robo_acq_eval(robo_gp* gp, int32_t acq_kind, double par, double eta, const double* Xc, int64_t m,
                      double* out_acq, double* out_max, int64_t* out_argmax, uint32_t* out_flags);
/* What the last argmax-only acquisition call on this handle did.  *out_outcome: */
#define ROBO_SCREEN_NOT_ELIGIBLE 0 /* the plain sweep ran: not an eligible call, or the factor is in its back-off   */
#define ROBO_SCREEN_SCREENED 1     /* out_n_survivors of out_n_screened candidates were solved                      */
#define ROBO_SCREEN_PROBE_USED 2   /* ... after the incumbent was taken from the exact values of the 128 candidates with the largest upper bounds */
#define ROBO_SCREEN_FELL_BACK 3    /* too many survivors (or none below the bound): the plain sweep ran on the whole batch */
int32_t robo_cand_last_screen(robo_cand* cand, int64_t* out_n_screened, int64_t* out_n_survivors, int32_t* out_outcome);
/* How the last bounds pass on this handle finished its covariances (tuning key acq_screen_lean): the fp64 finish selected
 * for the call, lean or full -- also when the single-precision first stage decided the call alone or supplied the bounds
 * (robo_cand_last_screen_first tells).  *out_finish: */
#define ROBO_SCREEN_FINISH_NONE 0  /* no bounds pass yet, or the direct-difference kernel (it has one finish)        */
#define ROBO_SCREEN_FINISH_FULL 1  /* the dot-form kernel, square root and exponential to the last bit               */
#define ROBO_SCREEN_FINISH_LEAN 2  /* the dot-form kernel, covariance to 8e-13 amp, that error in the margin           */
/* *out_fused_tail (may be NULL): 1 when the last argmax-only acquisition call on this handle ran its survivors' output
 * transform, acquisition, argmax, index map and report as the one single-workgroup launch (acq_screen_fused_tail), else 0. */
int32_t robo_cand_last_screen_finish(robo_cand* cand, int32_t* out_finish, int32_t* out_fused_tail);
/* The single-precision first stage of the last argmax-only acquisition call on this handle (tuning key acq_screen_single).
 * *out_stage: 0 it did not run (not an eligible call, the rule, its pause), 1 it decided the call: its survivors are the
 * ones robo_cand_last_screen counts as solved, 2 it ran and the fp64 pass followed on the whole batch.  *out_kept: the
 * first stage's survivor count (0 with stage 0).  Either pointer may be NULL.                                          */
int32_t robo_cand_last_screen_first(robo_cand* cand, int32_t* out_stage, int64_t* out_kept);
/* How that first stage -- of the last argmax-only acquisition call on this handle, or of the last robo_acq_screen_bounds
 * under acq_screen_single = 2 -- formed its squared distances (tuning key acq_screen_int).  *out_form:                   */
#define ROBO_SCREEN_FORM_FP64 0    /* no first stage, or |a|^2 + |b|^2 - 2 a.b from the fp64 matrix instruction           */
#define ROBO_SCREEN_FORM_INT8 1    /* exact int8 matrix products of the centred coordinates on a 24-bit grid              */
/* *out_step: the grid step in scaled coordinates (0 with ROBO_SCREEN_FORM_FP64).  Either pointer may be NULL.            */
int32_t robo_cand_last_screen_form(robo_cand* cand, int32_t* out_form, double* out_step);
/* The screen's bounds themselves (soundness tests, A/B tools): out_upper / out_lower (m,) with
 * lower <= the value robo_acq_eval_cand returns for the candidate <= upper; NaN coordinates give NaN bounds.  Needs a
 * (kind, par) the screen handles (LCB: kappa >= 0) and fp64 covariance entries; batch size, tuning keys and the
 * conditioning guard are not consulted.  The bounds are the fp64 pass's; with acq_screen_single = 2 (tests) they are the
 * single-precision first stage's wherever that stage may run.                                                        */
int32_t robo_acq_screen_bounds(robo_gp* gp, int32_t acq_kind, double par, double eta, robo_cand* cand, double* out_upper,
                               double* out_lower);
/* the element-wise half alone, for (mean, var) produced by any other BaseModel plugin
 * (the reference's acquisition classes accept every model, e.g. test/dummy_model.py)          */
int32_t robo_acq_eval_moments(robo_ctx* ctx, int32_t acq_kind, double par, double eta, const double* mean,
                              const double* var, int64_t m, double* out_acq, double* out_max, int64_t* out_argmax,
                              uint32_t* out_flags);
/* MarginalizationGPMCMC.compute (marginalization.py:115-121): mean over S fitted GPs of
 * the per-sample acquisition, accumulated in sample order (= NumPy's axis-0 mean).
 * etas (S): the incumbent value of every sample -- each estimator asks ITS OWN sub-model
 * (marginalization.py:40, ei.py:68): equal entries for plain GPs (observed minimum), different
 * ones for FabolasGP sub-models (predicted minimum of the projected points, fabolas_gp.py:141-164). */
int32_t robo_acq_eval_marginal_cand(robo_gp* const* gps, int32_t S, int32_t acq_kind, double par, const double* etas,
                                    robo_cand* cand, double* out_acq, double* out_max, int64_t* out_argmax,
                                    uint32_t* out_flags);
/* partial form for sample-sharded multi-GPU runs: returns sum_s acq_s (no division)          */
int32_t robo_acq_eval_sum_cand(robo_gp* const* gps, int32_t S, int32_t acq_kind, double par, const double* etas,
                               robo_cand* cand, double* out_acq_sum, uint32_t* out_flags);

/* ---- gradient refinement of the acquisition maximum (no counterpart in the reference, whose maximisers return a
 * candidate or run SciPy from the host): sweep over `cand` exactly as robo_acq_eval_cand, the n_starts (K <= 1024) best
 * candidates -- descending value, ties by ascending index, NaN never -- become the starts of K lock-step projected
 * gradient ascents in the box [0, 1]^dim of the GP's normalised input space, all on the device:
 *   evaluate value f and gradient g of the acquisition at the K points (D + 1 right-hand sides each: robo_gp_predict_grad's
 *   solve, one fused epilogue); n_steps times: g_proj = g with the components pointing out of the box at an active bound
 *   set to 0; |g_proj| = 0 -> the start is frozen; y = clip(x + alpha g_proj / |g_proj|, 0, 1); accept iff f(y) > f(x)
 *   (then x := y, alpha := min(2 alpha, 0.5)), else alpha := alpha / 2.  alpha starts at step0.  A trial whose variance
 *   sits on the floor or whose value is not finite freezes its start at the last accepted point (ROBO_FLAG_FROZEN).
 * Result: the start with the largest final value (first on ties): out_x (dim), *out_value, *out_start_index (its row in
 * `cand`; -1 when every candidate was NaN), *out_flags = the sweep's flags | ROBO_FLAG_FROZEN.  n_steps = 0 returns the
 * sweep's own argmax, point and value.  LogEI has a gradient here: d log EI = ds / s + (Phi / h)(z) dz, h = z Phi + phi.
 * Diagnostics (nullable): out_starts (n_starts) the rows the starts came from in selection order, -1 for unused slots
 * (fewer eligible candidates than n_starts); out_trace ((n_steps + 1) x n_starts x (2 dim + 3)): per iteration (0 = the
 * evaluation of the starts) and start the trial point, its value, its gradient, the step length it was made with, and
 * 1 / 0 / 2 / 3 = accepted / rejected / start frozen earlier (no trial made: the point is the start's own) / this
 * point has its variance on the floor or a value that is not finite (not taken; the start is frozen from here on).
 * One synchronisation per call; state and solve workspace stay with gp (gps[0]) between calls of one (n_starts, dim).  */
int32_t robo_acq_refine_cand(robo_gp* gp, int32_t acq_kind, double par, double eta, robo_cand* cand, int32_t n_starts,
                             int32_t n_steps, double step0, double* out_x, double* out_value, int64_t* out_start_index,
                             uint32_t* out_flags, int64_t* out_starts, double* out_trace);
/* the same for the mean over S fitted GPs (robo_acq_eval_marginal_cand's sweep): per sample the points are scaled with that
 * sample's length scales and solved against its factor; f and g are accumulated in sample order and divided by S.       */
int32_t robo_acq_refine_marginal_cand(robo_gp* const* gps, int32_t S, int32_t acq_kind, double par, const double* etas,
                                      robo_cand* cand, int32_t n_starts, int32_t n_steps, double step0, double* out_x,
                                      double* out_value, int64_t* out_start_index, uint32_t* out_flags,
                                      int64_t* out_starts, double* out_trace);

/* ---- entropy search's representer points: the ensemble sampler's whole run on the device (the reference drives emcee from
 * the host around one acquisition value per walker, robo/acquisition_functions/information_gain.py:132-151).  One chain of
 * n_walkers (k, even, >= 2 dim) walkers in the CALLER's input space samples exp(acquisition) of the fitted gp inside the box
 * [lower, upper] (a point with any coordinate < lower or > upper, or NaN, has log-probability -inf); normalize != 0: the
 * model's inputs are (x - lower) / (upper - lower).  Per half-step q = c - z (c - s), z = ((a - 1) u + 1)^2 / a (unfused,
 * NumPy's bits), the posterior of the k / 2 proposals exactly as robo_acq_eval forms it for a batch of that size, the
 * acquisition value as the log-density as it stands, and emcee 2's accept test (dim - 1) log z + lnp(q) - lnp(s) > log u.
 * u_stretch / partner / u_accept: [n_steps][2][k / 2], the draw order of robo_mcmc_draws.  pos (k, dim) and lnp (k) are
 * in-out; eval_start != 0: lnp is computed for the start positions, else taken as given.  out_accepted (k) counts the
 * accepted moves, out_flags is the OR of ROBO_FLAG_NEGATIVE_EI / ZERO_SIGMA / NAN over the chain's acquisition values.
 * out_trace (nullable): [n_steps][2][k / 2][dim + 2] = q, lnp(q), code 0 rejected / 1 accepted / 2 outside the box.
 * ROBO_BAD_ARGUMENT: odd k, k < 2 dim, lower >= upper, a partner outside [0, k / 2); ROBO_BAD_SHAPE: the k / 2 rows do not
 * fit the solve workspace (ws_bytes) -- the caller runs its host loop instead.  One synchronisation per call.             */
int32_t robo_rep_sample(robo_gp* gp, int32_t acq_kind, double par, double eta, const double* lower, const double* upper,
                        int32_t normalize, int32_t n_walkers, int32_t n_steps, double a, const double* u_stretch,
                        const int32_t* partner, const double* u_accept, double* pos, double* lnp, int32_t eval_start,
                        int64_t* out_accepted, uint32_t* out_flags, double* out_trace);
/* S independent chains in lock step, chain s against gps[s] (distinct fitted handles on one context with one N and dim) and
 * etas[s]; every per-chain array has a leading S axis.  Chain s equals robo_rep_sample on gps[s] bit for bit.             */
int32_t robo_rep_sample_batch(robo_gp* const* gps, int32_t S, int32_t acq_kind, double par, const double* etas,
                              const double* lower, const double* upper, int32_t normalize, int32_t n_walkers,
                              int32_t n_steps, double a, const double* u_stretch, const int32_t* partner,
                              const double* u_accept, double* pos, double* lnp, int32_t eval_start, int64_t* out_accepted,
                              uint32_t* out_flags, double* out_trace);

/* ---- greedy batch proposals with fantasised picks (no counterpart in the reference, which proposes one point per model
 * fit: robo/solver/bayesian_optimization.py:156-203).  q points are chosen from ONE candidate batch at FIXED theta, FIXED
 * constant mean and FIXED output transform (y_mean, y_std): nothing is re-estimated between the picks -- the result equals
 * appending every fantasy observation and refitting with those three frozen at the real data's values.
 * Pick 0 is robo_acq_eval_cand's sweep and argmax.  After pick j at candidate x_j a fantasy target y_f is chosen,
 *   ROBO_FANTASY_KRIGING_BELIEVER: y_f = mu(x_j) (per hyper-parameter sample in the marginal form),
 *   ROBO_FANTASY_CONSTANT_LIAR:    y_f = liar,
 * and every candidate's latent moments are conditioned on (x_j, y_f) observed with the model's noise:
 *   c(x) = cov(x, x_j | data and the earlier fantasies) = k(x, x_j) - k_*(x)^T beta_j - sum_{t<j} c_t(x) c_t(x_j) / d_t,
 *   beta_j = K^-1 k_*(x_j) (K: the fitted gram),  d = var_lat(x_j) + sigma^2 + 1.25e-12 (robo_gp_fit's diagonal),
 *   var_lat(x) -= c(x)^2 / d,   mu_lat(x) += c(x) (y_f - mu(x_j)) / d,   eta := min(eta, y_f)   (LCB ignores eta).
 * The state is kept unfloored in the latent scale; transform and DBL_EPSILON floor are applied when the acquisition is
 * formed, as in the sweep.  Nothing is masked: a picked point competes again with its collapsed variance.  beta_j always
 * comes from the two triangular solves with the factor, never from the explicit inverse W (no dependence on winv_cond_max).
 * A pick whose winning value is NaN is recorded and ends the selection: the remaining out_idx are -1, out_values /
 * out_fantasy NaN, and the call still succeeds.  *out_n_made = picks recorded.
 * out_idx / out_values / out_flags [q]: argmax (np.argmax: first index, NaN maximal), its value, the ROBO_FLAG_* of the
 * values the pick was made from.  out_fantasy [q] ([q][S] in the marginal form): the target fantasised at pick j (NaN for
 * the last pick made: nothing is conditioned on it).  out_trace, nullable, q x m x 2 (q x S x m x 2): the transformed,
 * floored (mean, var) every pick was made from -- diagnostics.  q outside 1 .. min(m, 1024) (the history of the
 * conditioning steps is S x q x m doubles), an unknown fantasy_kind, or a GP with
 * fp32 covariance entries: ROBO_BAD_ARGUMENT.  q = 1 is robo_acq_eval_cand / robo_acq_eval_marginal_cand bit for bit.
 * One synchronisation per call; the state stays with gp (gps[0]) between calls of one (m, S).                          */
enum robo_fantasy_kind { ROBO_FANTASY_KRIGING_BELIEVER = 0, ROBO_FANTASY_CONSTANT_LIAR = 1 };
int32_t robo_acq_batch_cand(robo_gp* gp, int32_t acq_kind, double par, double eta, robo_cand* cand, int32_t q,
                            int32_t fantasy_kind, double liar, int64_t* out_idx, double* out_values, double* out_fantasy,
                            uint32_t* out_flags, int32_t* out_n_made, double* out_trace);
int32_t robo_acq_batch_marginal_cand(robo_gp* const* gps, int32_t S, int32_t acq_kind, double par, const double* etas,
                                     robo_cand* cand, int32_t q, int32_t fantasy_kind, double liar, int64_t* out_idx,
                                     double* out_values, double* out_fantasy, uint32_t* out_flags, int32_t* out_n_made,
                                     double* out_trace);

/* ---- joint Monte-Carlo batch EI (q-EI) with greedy picks (no counterpart in the reference).  What the fantasies above stand
 * in for:  qEI(x_0 .. x_{q-1}) = E[(eta - par - min_t f(x_t))^+]  under the joint posterior of the q points, estimated over
 * K scenarios and maximised greedily over ONE candidate batch.  Greedy selection is exact for the estimate: with
 * b^k = min(eta - par, f^k(picks so far)) in scenario k,  qEI(picks, x) = qEI(picks) + E[(b - f(x))^+], so pick j maximises
 * the increment and the increments (out_gain) sum to the batch's q-EI estimate.  The innermost normal is integrated in
 * closed form, so a term is plain EI with a per-scenario shifted mean and incumbent.  EI only: LogEI, PI and LCB have no
 * joint form here (the mean of logs over hyper-parameter samples is not the log of the mean).
 * Everything is per hyper-parameter sample s, in the latent scale, at FIXED theta, constant mean and output transform.
 * z: K x q row-major finite doubles, standard-normal base samples shared by all hyper-parameter samples; z[k][t] drives
 * pick t in scenario k.  eps = DBL_EPSILON.
 * Pick 0 is robo_acq_eval_cand's (robo_acq_eval_marginal_cand's) EI sweep and argmax, launch for launch; after it
 * b^k := eta_s - par (one rounded subtraction) for all k.
 * After pick t at candidate p_t -- no noise term and no jitter, a pick is not an observation --
 *   c_t(x) = k(x, p_t) - k_*(x)^T beta_t - sum_{u<t} c_u(x) c_u(p_t) / d_u,   beta_t = K^-1 k_*(p_t) (the two triangular
 *            solves, never the explicit inverse W),
 *   d_t = max(var_lat(p_t), eps / y_std^2)   (var_lat(p_t): the residual variance before this step; NaN propagates),
 *   l_t(x) = c_t(x) / sqrt(d_t),   var_lat(x) -= l_t(x)^2;   mu_lat is never touched,
 *   f^k(p_t) = mean_t(p_t) + y_std (sum_{u<t} l_u(p_t) z[k][u] + sqrt(d_t) z[k][t]),   b^k := min(b^k, f^k(p_t))
 *            (u ascending, products fused into the sum, the outer product-sum one fma; a NaN f^k makes b^k NaN).
 * Value of candidate x at pick j >= 1:
 *   g_s(x) = (1/K) sum_k EI(mean_t(x) + y_std sum_{u<j} l_u(x) z[k][u], max(var_lat(x) y_std^2, eps), b^k, 0)
 * with robo_acq_eval's EI, its +0 for a term in (-DBL_MIN, 0) and its flags.  The K terms are summed in FOUR groups of
 * ceil(K / 4) consecutive scenarios (group w starts at k = w ceil(K / 4)), each with k ascending from +0, combined as
 * ((G0 + G1) + (G2 + G3)) / K: the grouping depends on K alone -- not on m, the candidate's position or the grid -- so a
 * candidate's value has the same bits at any batch position.  The marginal form averages g_s over the samples in sample
 * order.  The winner follows np.argmax (first index, NaN maximal).  A NaN winner is recorded and ends the selection as in
 * robo_acq_batch_cand: the remaining out_idx are -1, out_gain NaN.  Nothing is masked.
 * out_idx / out_gain / out_flags [q]: the pick, its value (the running sum of gains is the batch's q-EI estimate), the
 * ROBO_FLAG_* of the values it was made from; *out_n_made = picks recorded.  Diagnostics, all nullable; rows of picks that
 * were not made are NaN:
 *   out_acq   q x m            every candidate's value at every pick
 *   out_trace q x S x m x 2    the transformed mean and the transformed, floored residual variance every pick was made from
 *   out_coef  (q-1) x S x m    c_t(x)
 *   out_d     q x S            d_t (NaN for the last pick made: nothing is conditioned on it)
 *   out_best  q x S x K        the b^k every pick was made from
 * ROBO_BAD_ARGUMENT with a message: q outside 1 .. min(m, ROBO_QEI_MAX_Q), K outside 1 .. ROBO_QEI_MAX_K, z NULL or not
 * finite (also for q = 1, which does not use it), an unfitted GP, a GP with fp32 covariance entries, samples that do not
 * match the candidates or each other (what robo_acq_batch_marginal_cand refuses).  q = 1 is robo_acq_eval_cand(EI) bit
 * for bit.  One synchronisation per call; the state stays with gp (gps[0]) between calls of one (m, S, q, K).  Event slots
 * 30 and 31 bracket the fold kernel of the last pick (last sample), under the condition of slots 24..27.            */
#define ROBO_QEI_MAX_Q 64
#define ROBO_QEI_MAX_K 1024
int32_t robo_qei_batch_cand(robo_gp* gp, double par, double eta, robo_cand* cand, int32_t q, const double* z, int32_t K,
                            int64_t* out_idx, double* out_gain, uint32_t* out_flags, int32_t* out_n_made, double* out_acq,
                            double* out_trace, double* out_coef, double* out_d, double* out_best);
int32_t robo_qei_batch_marginal_cand(robo_gp* const* gps, int32_t S, double par, const double* etas, robo_cand* cand,
                                     int32_t q, const double* z, int32_t K, int64_t* out_idx, double* out_gain,
                                     uint32_t* out_flags, int32_t* out_n_made, double* out_acq, double* out_trace,
                                     double* out_coef, double* out_d, double* out_best);

/* ---- max-value entropy search (Wang & Jegelka, ICML 2017; no counterpart in the reference), for minimisation.
 * Inputs are the sweep's transformed, floored moments (mu_i, v_i) of the m candidates (what robo_gp_predict_cand returns),
 * sigma_i = sqrt(v_i).  F(w) = sum_i log Phi((w + mu_i) / sigma_i) is the log-probability that max_i(-f_i) < w for
 * independent f_i (a candidate with sigma_i == 0 is a step: -inf for w < -mu_i, else 0).
 *   bracket    w_lo = max_i(-mu_i - 8 sigma_i), w_hi = max_i(-mu_i + 8 sigma_i):  F(w_lo) <= log Phi(-8) < log 1/4 and
 *              F(w_hi) >= m log Phi(8) > log 3/4 for every m a handle can hold -- no bracket search.
 *   quantiles  w_p solves F(w_p) = log p for p = 1/4, 1/2, 3/4: a sectioning search on the device (64 sections per pass,
 *              all three quantiles per pass over the candidates, no host round trip) until every quantile's bracket is no
 *              wider than max((w_hi - w_lo) 2^-46, 4 ulp of its larger end); w_p is the bracket's midpoint.
 *   Gumbel fit b = (w_1/4 - w_3/4) / (log log(4/3) - log log 4),  a = w_1/2 + b log log 2.
 *   draws      y*_k = -(a - b log(-log u_k)) for the CALLER's u_k in (0, 1), k < K, 1 <= K <= 128; with clamp != 0
 *              y*_k := min(y*_k, eta).
 *   value      alpha_i = (1/K) sum_k [ gamma phi(gamma) / (2 Phi(gamma)) - log Phi(gamma) ],  gamma = (mu_i - y*_k) / sigma_i,
 *              summed in ascending k, phi / Phi = exp(log phi - log Phi); a term's 0 * inf (huge gamma) counts as 0.
 *              sigma_i == 0: alpha_i = 0 and ROBO_FLAG_ZERO_SIGMA;  a NaN moment: alpha_i = NaN and ROBO_FLAG_NAN.
 *              Accuracy: for gamma >= 0 a term is good to a few ulp.  For gamma < 0 it is the difference of two numbers
 *              near gamma^2 / 2 that leaves ~log(-gamma) + 1.4: its relative error is about gamma^2 eps / (2 log(-gamma))
 *              -- 3e-14 at gamma = -30 (the tested range), 1e-9 at -1e4, no digits beyond about -1e8, and NaN
 *              (inf - inf, flagged) beyond |gamma| ~ 1e154.  With clamp != 0 every y* <= eta, so gamma < 0 occurs only
 *              where a candidate's mean lies below the incumbent, and |gamma| <= (eta - mu_i) / sigma_i.
 * Every sum has a fixed order (128 candidates per partial in index order, partials in block order): two calls on the same
 * inputs return the same bits.  argmax follows np.argmax (first index, NaN maximal) through the sweep's own reduction.
 * Diagnostics, all nullable: out_ystar (K), out_gumbel (7: w_lo, w_hi, w_1/4, w_1/2, w_3/4, a, b), out_trace (m x 2: the
 * (mean, var) the call worked on).  out_acq (m) may be NULL.  A u outside the open interval (0, 1), K outside 1 .. 128, a GP
 * that is not fitted, or a NaN moment in the sampling half: ROBO_BAD_ARGUMENT.
 * One synchronisation per call; the state stays with gp (gps[0]) between calls of one (m, S, K).  Event slots 30 and 31
 * are recorded behind the minimum sampling and the element-wise half of the last sample, under the condition of slots
 * 24..27 (27 -> 30 -> 31: the tail's two phases).                                                                        */
int32_t robo_mes_eval_cand(robo_gp* gp, double eta, robo_cand* cand, const double* u, int32_t K, int32_t clamp,
                           double* out_acq, double* out_max, int64_t* out_argmax, uint32_t* out_flags, double* out_ystar,
                           double* out_gumbel, double* out_trace);
/* the mean over S fitted GPs: every sample runs its own sweep, bracket, quantiles, Gumbel fit and y*_{s,k} from u[s][k]
 * (clamped to its own etas[s]); alpha = (sum_s alpha_s) / S accumulated in sample order, as robo_acq_eval_marginal_cand.
 * u and out_ystar S x K, out_gumbel S x 7, out_trace S x m x 2.                                                           */
int32_t robo_mes_eval_marginal_cand(robo_gp* const* gps, int32_t S, const double* etas, robo_cand* cand, const double* u,
                                    int32_t K, int32_t clamp, double* out_acq, double* out_max, int64_t* out_argmax,
                                    uint32_t* out_flags, double* out_ystar, double* out_gumbel, double* out_trace);
/* the two halves on their own, for (mean, var) produced by any other BaseModel plugin (as robo_acq_eval_moments):
 * the sampling half (bracket, quantiles, Gumbel fit, draws) over a discretisation's moments ...                          */
int32_t robo_mes_sample_min_moments(robo_ctx* ctx, const double* mean, const double* var, int64_t m, const double* u,
                                    int32_t K, int32_t clamp, double eta, double* out_ystar, double* out_gumbel);
/* ... and the element-wise half with its argmax for given y* (K)                                                         */
int32_t robo_mes_eval_moments(robo_ctx* ctx, const double* mean, const double* var, int64_t m, const double* ystar,
                              int32_t K, double* out_acq, double* out_max, int64_t* out_argmax, uint32_t* out_flags);

/* ---- knowledge gradient over a discretisation (Frazier, Powell & Dayanik 2009; no counterpart in the reference), for
 * minimisation: how much the MINIMUM OF THE POSTERIOR MEAN is expected to drop after one more noisy observation at x.
 * The discretisation A = {z_0 .. z_{nb-1}} is a candidate handle `rep` in the model's normalised input space,
 * 1 <= nb <= 64: the representer handle of robo_ig_eval_cand, its solve cached across calls in the same way (while the
 * factor and the points stay the same).  For a candidate x:
 *   a_j     = mu(z_j), the transformed posterior mean of the discretisation (what robo_gp_predict_cand returns for rep),
 *             computed on the device by the call
 *   v       = var(x), the sweep's transformed variance, floored at DBL_EPSILON as it stands
 *   s_j     = y_std^2 (k(x, z_j) - v_x . v_zj), the posterior covariance, SIGNED and not floored (robo_gp_cross_cov clips
 *             at DBL_EPSILON because the reference does; the knowledge gradient needs the sign)
 *   sigma~  = sqrt(v + sn2), sn2 >= 0 in the scale of the returned variances, as robo_ig_eval_cand takes it
 *   b_j     = s_j / sigma~, the slopes;  include_self != 0: one more line for x itself, a_nb = mu(x), b_nb = v / sigma~,
 *             n = nb + 1 <= 65 lines, otherwise n = nb
 *   KG(x)   = min_j a_j - E_Z[ min_j (a_j + b_j Z) ],  Z ~ N(0, 1),  KG(x) >= 0.
 * Evaluated in the envelope form, in which every term is non-negative (the direct form sum_j a_j (Phi(hi_j) - Phi(lo_j))
 * + ... subtracts numbers of size |a| to obtain a result that may be 1e-12 |a|; it is not used):
 *   1. A_j = -a_j, B_j = -b_j.
 *   2. The lines are ordered by (B ascending, A descending, index ascending).
 *   3. Of lines with equal B only the first is kept.
 *   4. Upper-envelope stack scan: for the next line i and the stack top t, c = (A_t - A_i) / (B_i - B_t); while c <= the
 *      breakpoint stored with t, t is popped; then i is pushed with breakpoint c.  The bottom line's breakpoint is -inf.
 *   5. KG = sum_k (B_k - B_{k-1}) f(-|c_k|) over consecutive survivors, in ascending k, with
 *      f(-t) = phi(t) (1 - t sqrt(pi/2) erfcx(t / sqrt 2)).  A term with |c_k| > 36 counts as exactly 0 (its true size is
 *      below 1e-283 (B_k - B_{k-1}); phi is subnormal from about 37.6).  A term's own conditioning is eps (t^2 + 1).
 * A NaN among v, mu(x), any s_j or any a_j: KG = NaN and ROBO_FLAG_NAN.  A single surviving line: exactly 0.0.  Every sum
 * and the sort have a fixed order: two calls on the same inputs, and the same candidate at any batch position, give the
 * same bits.  argmax follows np.argmax (first index, NaN maximal) through the sweep's own reduction.
 * out_kg (m) and out_disc_mean (nb: the a_j) are nullable; out_trace, nullable, m x (nb + 2): per candidate
 * s_0 .. s_{nb-1}, v, mu(x) as the kernel read them -- the inputs from which an oracle can recompute the value.
 * nb outside 1 .. 64, sn2 < 0 or NaN, a NULL required pointer, a GP with fp32 covariance entries: ROBO_BAD_ARGUMENT; a GP
 * that is not fitted: ROBO_NOT_FITTED; cand and rep on different contexts or of different dim: ROBO_BAD_SHAPE.
 * One synchronisation per call.  Event slots 30 and 31 bracket the envelope kernel of the last sample, under the
 * condition of slots 24..27.                                                                                        */
int32_t robo_kg_eval_cand(robo_gp* gp, robo_cand* cand, robo_cand* rep, double sn2, int32_t include_self, double* out_kg,
                          double* out_max, int64_t* out_argmax, uint32_t* out_flags, double* out_disc_mean,
                          double* out_trace);
/* the mean over S fitted GPs: sample s is taken against gps[s] and sn2s[s] with the shared rep, re-solved per sample;
 * KG = (sum_s KG_s) / S accumulated in sample order, as robo_acq_eval_marginal_cand.  out_disc_mean S x nb, out_trace
 * S x m x (nb + 2).  S = 1 equals the single form bit for bit.                                                      */
int32_t robo_kg_eval_marginal_cand(robo_gp* const* gps, int32_t S, robo_cand* cand, robo_cand* rep, const double* sn2s,
                                   int32_t include_self, double* out_kg, double* out_max, int64_t* out_argmax,
                                   uint32_t* out_flags, double* out_disc_mean, double* out_trace);
/* the envelope kernel alone for any model's moments (as robo_ig_eval_moments): s (m, nb) signed covariances, v (m),
 * mean (m), disc_mean (nb).  Equals the fused call bit for bit when fed the fused call's own trace.                  */
int32_t robo_kg_eval_moments(robo_ctx* ctx, int64_t m, int32_t nb, double sn2, int32_t include_self, const double* s,
                             const double* v, const double* mean, const double* disc_mean, double* out_kg,
                             double* out_max, int64_t* out_argmax, uint32_t* out_flags);

/* ---- two-objective expected hypervolume improvement (Emmerich, Deutz & Klinkenberg 2011, for minimisation; not in the
 * reference): the expected gain in dominated hypervolume of one more observation whose two objectives have independent
 * normal posteriors.  ref = (r1, r2) is the reference point; front (P x 2, row-major) holds 0 <= P <= ROBO_EHVI_MAX_FRONT
 * mutually non-dominated points (a_i, b_i), i = 1 .. P, every one strictly below ref in both coordinates, sorted with a
 * strictly ascending, hence b strictly descending.  With the sentinels a_0 = -inf, a_{P+1} = r1, b_0 = r2 the region inside
 * ref that the front does not dominate is the union of the strips [a_i, a_{i+1}) x (-inf, b_i), i = 0 .. P, and for
 * y1 ~ N(mu1, s1^2), y2 ~ N(mu2, s2^2):
 *   g(b; mu, s) = E[(b - y)^+] = s f((b - mu) / s),  f(z) = phi(z) + z Phi(z),  g(-inf) = 0;  s == 0: max(b - mu, 0)
 *   EHVI        = sum_{i=0}^{P} [ g(a_{i+1}; mu1, s1) - g(a_i; mu1, s1) ] g(b_i; mu2, s2),  every term >= 0.
 * f is taken as f(z) = max(z, 0) + f(-|z|) with the knowledge gradient's erfcx form of f(-t) above: it carries only its own
 * conditioning eps (z^2 + 1) and is exactly 0 for z < -36.  The strips are summed in index order i = 0 .. P, the boundary
 * value g(a_i) carried from strip to strip (P + 2 evaluations of g for objective 1, P + 1 for objective 2), by a
 * compensated (Kahan) sum, so that the accumulation costs 2 eps of the sum whatever P is; a difference of two rounded g
 * values that comes out negative counts as 0.  Every operation is rounded once and never contracted, and the order depends
 * on nothing but the front: the same four moments give the same bits at any batch position, for any m, any chunking and
 * in either entry point.
 * A NaN among the four moments (or a negative variance): EHVI = NaN and ROBO_FLAG_NAN.  s1 == 0 or s2 == 0: ROBO_FLAG_ZERO_SIGMA, the value by the
 * max branch (not zeroed).  argmax follows np.argmax (first index, NaN maximal) through the sweep's own reduction.
 * The fused form runs the sweep of gp1 over cand, keeps its moments, runs the sweep of gp2, then the strip kernel and the
 * reduction, with one synchronisation; both sweeps are chunked by the candidate workspace.  The moments are what
 * robo_gp_predict_cand returns (output transform applied, variance floored at DBL_EPSILON), so the two GPs may differ in
 * kernel, hyper-parameters, N and output normalisation.  out_ehvi (m) is nullable; out_trace, nullable, m x 4: per candidate
 * mean1, var1, mean2, var2 as the kernel read them.  Later calls on the same handles return what they return on fresh ones.
 * P outside 0 .. ROBO_EHVI_MAX_FRONT, a non-finite ref or front entry, a front that is not sorted as above or has a point
 * not strictly below ref, a NULL required pointer, GPs or cand on different contexts: ROBO_BAD_ARGUMENT; a GP whose dim
 * is not cand's: ROBO_BAD_SHAPE; a GP that is not fitted: ROBO_NOT_FITTED -- all before anything is launched.
 * Event slots 30 and 31 bracket the strip kernel, under the condition of slots 24..27.                              */
#define ROBO_EHVI_MAX_FRONT 4096
int32_t robo_ehvi_eval_cand(robo_gp* gp1, robo_gp* gp2, robo_cand* cand, const double* front, int32_t P, const double* ref,
                            double* out_ehvi, double* out_max, int64_t* out_argmax, uint32_t* out_flags,
                            double* out_trace);
/* the strip kernel alone for any model's moments: mean1, var1, mean2, var2 (m each).  Equals the fused call bit for bit
 * when fed the fused call's own trace.                                                                              */
int32_t robo_ehvi_eval_moments(robo_ctx* ctx, int64_t m, const double* mean1, const double* var1, const double* mean2,
                               const double* var2, const double* front, int32_t P, const double* ref, double* out_ehvi,
                               double* out_max, int64_t* out_argmax, uint32_t* out_flags);

/* ---- constrained expected improvement (Schonlau, Welch & Jones 1998; Gardner et al. 2014; Gelbart, Snoek & Adams 2014; not
 * in the reference): expected improvement weighted by the probability that C black-box constraints hold, each modelled by a
 * GP of its own.
 *   Inputs.     The objective's posterior N(mu_0, s_0^2) and C constraints with independent posteriors N(mu_k, s_k^2),
 *               k = 1 .. C, 0 <= C <= ROBO_CEI_MAX_CONSTRAINTS; thresholds t_k.  Constraint k holds when c_k(x) <= t_k, in the
 *               scale robo_gp_predict_cand returns (output transform applied).
 *   Per candidate.   z_k = (t_k - mu_k) / s_k,   L = sum_{k=1..C} norm_logcdf(z_k) summed in index order from 0,
 *               PoF = exp(L).  norm_logcdf is the plain sweep's log Phi (erfcx form for z < -1: L stays finite where Phi has
 *               long underflowed; log1p form otherwise).
 *   Value.      acq_kind         has_eta   value
 *               ROBO_ACQ_EI      1         EI(mu_0, var_0, eta, par) * PoF
 *               ROBO_ACQ_LOG_EI  1         LogEI(mu_0, var_0, eta, par) + L
 *               ROBO_ACQ_EI      0         PoF
 *               ROBO_ACQ_LOG_EI  0         L
 *               has_eta = 0 says that no feasible observation exists yet: eta and par are ignored.  The objective factor comes
 *               from the device functions of robo_acq_eval_cand with the same guards (an EI in (-DBL_MIN, 0) is +0), so with
 *               C = 0 and has_eta = 1 the call returns robo_acq_eval_cand's bits.  Any other acq_kind: ROBO_BAD_ARGUMENT.
 *   Arithmetic. The difference, the quotient, every addition of the sum and the final product or addition are rounded once
 *               and never contracted, and their order depends on nothing but C: a value's bits do not depend on the batch
 *               position, on m, on the chunking or on which of the two entry points produced it.
 *   Edges.      s_k == 0 (the moments form only: the fused form's variances are floored at DBL_EPSILON): the constraint's
 *               factor is 1 (log factor 0) if mu_k <= t_k, else 0 (log factor -inf), and ROBO_FLAG_ZERO_SIGMA.  s_0 == 0 with
 *               has_eta = 1 is handled by the objective functions' own branches and raises the same flag.  A NaN among the
 *               2 (C + 1) moments, or a negative variance, gives NaN and ROBO_FLAG_NAN (the objective's moments count with
 *               has_eta = 0 too).  A negative EI raises ROBO_FLAG_NEGATIVE_EI as in robo_acq_eval_cand.  argmax follows
 *               np.argmax (first index, NaN maximal) through the sweep's own reduction.
 * The fused form runs the C + 1 sweeps over cand, each chunked by the candidate workspace, into the rows of the handle's sample
 * tables, then the fold kernel, the reduction and the read-back with one synchronisation.  The GPs may differ in kernel kind,
 * hyper-parameters, N and output normalisation.  out_values (m) is nullable; out_trace, nullable, m x (2 (C + 1) + 2): per
 * candidate mu_0, var_0, mu_1, var_1, .. mu_C, var_C as the kernel read them, then L and the objective factor (1 resp. 0 with
 * has_eta = 0).  Later calls on the same handles return what they return on fresh ones.
 * C out of range, a NULL required pointer, a non-finite threshold, has_eta = 1 with a non-finite eta or par, GPs or cand on
 * different contexts: ROBO_BAD_ARGUMENT; a GP whose dim is not cand's: ROBO_BAD_SHAPE; a GP that is not fitted:
 * ROBO_NOT_FITTED -- all before anything is launched.
 * Event slots 32 and 33 bracket the fold kernel, under the condition of slots 24..27.                                  */
#define ROBO_CEI_MAX_CONSTRAINTS 16
int32_t robo_cei_eval_cand(robo_gp* objective, robo_gp* const* constraints, int32_t C, const double* thresholds,
                           int32_t acq_kind, double par, double eta, int32_t has_eta, robo_cand* cand,
                           double* out_values /* nullable */, double* out_max, int64_t* out_argmax, uint32_t* out_flags,
                           double* out_trace /* nullable */);
/* ---- gradient refinement of the constrained value: robo_acq_refine_cand's multi-start projected ascent on the value of
 * robo_cei_eval_cand.  The constrained optimum usually lies on a constraint boundary, which random candidates only straddle.
 *   Sweep.      Exactly robo_cei_eval_cand's without values read back: the same arguments, the same checks, the same values
 *               left in the handle.
 *   Starts, ascent, result, trace.   Exactly robo_acq_refine_cand's: the n_starts (K <= 1024) best candidates in descending
 *               value, ties by ascending index, NaN never; projected unit-length steps in [0, 1]^dim; accept iff f(y) > f(x);
 *               alpha doubles up to 0.5 or halves; a start freezes (ROBO_FLAG_FROZEN) when a trial's variance sits on the
 *               floor, its value is not finite or no direction is left; out_trace ((n_steps + 1) x n_starts x (2 dim + 3)) has
 *               the same columns and codes 0 / 1 / 2 / 3; n_steps = 0 returns the sweep's own argmax, point and value; one
 *               synchronisation per call.
 *   Value at a trial point.   The fold's rule on the moments the (dim + 1)-row solve gives for that point: per GP m, v, dm, dv
 *               as robo_acq_refine_cand forms them, the variance floored at DBL_EPSILON -- the floor in ANY of the GPs solved
 *               marks the trial (code 3).  z_k = (t_k - m_k) / s_k and the sum L of norm_logcdf(z_k) in index order from 0,
 *               each operation rounded once; value = f0 (C = 0), f0 + L (LogEI), f0 * exp(L) (EI), rounded once, with f0 the
 *               objective factor of robo_acq_refine_cand (EI's guard included); has_eta = 0: L resp. exp(L).
 *   Gradient.   dz_k = (-dm_k - z_k ds_k) / s_k, ds = dv / (2 s); dl_k = r(z_k) dz_k, r = phi / Phi as the plain quotient for
 *               z >= -1 and 1 / (sqrt(pi / 2) erfcx(-z / sqrt 2)) below, which is finite wherever L is; dL summed in index
 *               order.  With g0 the objective's gradient (robo_acq_refine_cand's formulas): g0 + dL (LogEI),
 *               exp(L) (g0 + f0 dL) (EI); has_eta = 0: dL resp. exp(L) dL.  The gradient carries no bit contract; the value's
 *               last operation, the accept test, the step-length update, the trial point and its clip are single rounded
 *               operations on stored doubles.
 *   Order.      Per trial the GPs are solved one after the other, constraints 1 .. C first, the objective last; its epilogue
 *               combines, decides and writes the next trial.  With has_eta = 0 the iterations leave the objective's GP out
 *               entirely (only the sweep reads it) and the last constraint's epilogue decides; with C = 0 as well the value is
 *               constant and every start freezes after its evaluation.
 *   Consequences.   With C = 0 and has_eta = 1 the call returns robo_acq_refine_cand's result and trace bit for bit.  A start's
 *               trajectory does not depend on n_starts or on its slot.  In the product form (EI) a start whose value has
 *               underflowed to 0 has a zero gradient, hence no direction, and freezes: the log form (LogEI) is the one that
 *               climbs out of infeasible regions.
 * The GPs may differ in kernel kind (Matern-5/2, RBF), hyper-parameters, N and output normalisation; each is solved through
 * the explicit inverse or by block rows by the library's rule for its own factor.  A Fabolas kernel: ROBO_BAD_ARGUMENT (its
 * fidelity column is not a box coordinate).  n_starts, n_steps, step0 out of range: ROBO_BAD_ARGUMENT; n_starts (dim + 1)
 * rows of the LARGEST n_pad among the GPs the iterations solve exceeding the solve workspace: ROBO_BAD_SHAPE; otherwise
 * robo_cei_eval_cand's refusals -- all before anything is launched.  State and workspace stay with `objective` (shared with
 * robo_acq_refine_cand on it).  No event slot of its own: the sweep records 32 and 33 as robo_cei_eval_cand does.        */
int32_t robo_cei_refine_cand(robo_gp* objective, robo_gp* const* constraints, int32_t C, const double* thresholds,
                             int32_t acq_kind, double par, double eta, int32_t has_eta, robo_cand* cand,
                             int32_t n_starts, int32_t n_steps, double step0,
                             double* out_x, double* out_value, int64_t* out_start_index, uint32_t* out_flags,
                             int64_t* out_starts /* nullable */, double* out_trace /* nullable */);
/* the fold kernel alone for any models' moments: mean0, var0 (m), means, vars (C x m, row-major, row k = constraint k + 1;
 * not read when C = 0).  Equals the fused call bit for bit when fed the fused call's own trace.                          */
int32_t robo_cei_eval_moments(robo_ctx* ctx, int64_t m, int32_t C, const double* mean0, const double* var0,
                              const double* means, const double* vars, const double* thresholds, int32_t acq_kind,
                              double par, double eta, int32_t has_eta, double* out_values, double* out_max,
                              int64_t* out_argmax, uint32_t* out_flags);

/* ---- pathwise posterior samples (Matheron's rule; Wilson et al. 2020, "Efficiently sampling functions from Gaussian
 * process posteriors"; not in the reference): S whole functions drawn from the posterior of one fitted GP, evaluated and
 * minimised over candidate batches of any size -- Thompson sampling, and S parallel proposals from one call.
 *   f_s(x) = c + phi(x) . w_s + k(x, X) . alpha_s,     alpha_s = (K + noise I)^-1 (y - c - Phi_X w_s - sqrt(noise) eps_s)
 * All inputs are in the GP's scaled space: x~ = x (.) ism with ism the inverse square-root metric scale_inputs_kernel
 * applies.  Kernel kinds ROBO_KERNEL_MATERN52_ARD and ROBO_KERNEL_RBF_ARD only.
 *   Features.   phi_f(x) = sqrt(2 amp / F) cos(x~ . omega_f + b_f), f = 0 .. F - 1.  The caller gives omega (F x D,
 *               row-major), phase b (F) and the standard-normal draws w (S x F) and eps (S x N).  The library draws nothing:
 *               the result is a deterministic function of its arguments.
 *   Right-hand side.  r_s = (y - c) - Phi_X w_s - sqrt(noise + JITTER) eps_s, with y, c and the noise exactly what the fit
 *               used (y after the output normalisation, noise + JITTER the fit's diagonal addition); Phi_X is phi at the
 *               training rows, evaluated by the kernel that later evaluates candidates.
 *   Weights.    alpha_s = L^-T L^-1 r_s with the factor the GP holds, by forward and backward block rows with the fit's
 *               inverted diagonal blocks, followed by ONE step of iterative refinement against K itself with the same factor:
 *               rho_s = r_s - (K alpha_s + (noise + JITTER) alpha_s), alpha_s += L^-T L^-1 rho_s, K alpha_s at the training
 *               rows formed by the path kernel (diagonal entries exactly amp).  alpha is large where the noise is small
 *               (like sqrt(N) / noise against values of O(1)), so the few ulps by which the factor's K differs from the
 *               kernel's own entries would otherwise reach the values.  A path's weights are formed by the same
 *               operations whatever S is.
 *   Value.      f_s(x) = c + sum_f phi_f(x) w_sf + sum_j k(x~, X~_j) alpha_sj, then the output transform of
 *               robo_gp_predict_cand (f y_std + y_mean).  One accumulator per (x, s) takes the training points in tiles of 64 in
 *               index order, then the features in tiles of 64 in index order, each product on the fp64 matrix pipe; k is
 *               formed from |x~|^2 + |X~_j|^2 - 2 x~ . X~_j (clamped at 0).  Consequently the bits of f_s(x) depend only on x,
 *               the GP and path s's own draws: not on the candidate's position in the batch, on m, on the chunking, on S or
 *               on the other paths' draws.
 *   Pick.       Per path np.argmax(-f_s): first index, NaN maximal; out_min[s] is f_s at the pick.
 *   NaN.        A NaN coordinate of a candidate gives NaN in every path at that candidate and ROBO_FLAG_NAN.
 * robo_paths_create is one call with one synchronisation.  The object is a SNAPSHOT: it keeps the scaled training rows, the
 * metric, alpha, omega, b, w, the amplitude, the kind, c and the output transform.  Later fits, robo_gp_set_data or the
 * destruction of the GP do not change a paths object.  Kind ROBO_KERNEL_FABOLAS (the kernel is not stationary), F outside
 * 1 .. ROBO_PATHS_MAX_FEATURES, S outside 1 .. ROBO_PATHS_MAX, a NULL pointer, a non-finite entry of omega, phase, w or
 * eps: ROBO_BAD_ARGUMENT; a GP that is not fitted: ROBO_NOT_FITTED -- all before anything is launched.
 * robo_paths_eval_cand is one call with one synchronisation, chunked by the candidate workspace (S x chunk values) when the
 * values are asked for, a per-path best carried across the chunks.  out_values (S x m, row-major) is nullable, out_min (S),
 * out_argmin (S) and out_flags are not.  cand's dim is not the GP's: ROBO_BAD_SHAPE; cand on another context or a NULL
 * pointer: ROBO_BAD_ARGUMENT.  robo_paths_destroy(NULL) is harmless.  Event slots 30 and 31 bracket the passes of the path
 * kernel (with the values' copies in between when they are asked for), under the condition of slots 24..27.               */
#define ROBO_PATHS_MAX 64             /* S */
#define ROBO_PATHS_MAX_FEATURES 4096  /* F */
typedef struct robo_paths robo_paths; /* S posterior sample paths of one fitted GP (a snapshot) */
int32_t robo_paths_create(robo_gp* gp, int32_t F, int32_t S, const double* omega, const double* phase,
                          const double* w, const double* eps, robo_paths** out);
int32_t robo_paths_eval_cand(robo_paths* p, robo_cand* cand, double* out_values /* S x m, nullable */,
                             double* out_min /* S */, int64_t* out_argmin /* S */, uint32_t* out_flags);
int32_t robo_paths_destroy(robo_paths* p);

/* ---- refinement of a path's minimiser: multi-start projected gradient descent on the paths themselves, all descents of all
 * paths in ONE launch (paths_refine.hip).  A path is a closed-form differentiable function: its value and gradient at a point
 * need no solve and depend on nothing but that point.
 *   Space.      Coordinates are in the GP's normalised input space, box [0, 1]^dim, as for robo_acq_refine_cand.
 *   Value.      With x~ = x (.) ism (one rounding per coordinate, as scale_inputs_kernel), the value is the one above:
 *               f_s(x) = (c + sum_f phi_f w_sf + sum_j k(x~, X~_j) alpha_sj) y_std + y_mean, with k formed from the squared
 *               distance in the DIFFERENCE form sum_d (x~_d - X~_jd)^2 (cross_grad_kernel's).  These values are NOT
 *               robo_paths_eval_cand's bits, which come off the matrix pipe in the dot form: a descent compares values of its
 *               own kernel only, and the two agree within the bound of the path values (tests/test_paths_refine.py).
 *   Gradient.   d f_s / d x_d = y_std ism_d [ -fscale sum_f w_sf sin(x~ . omega_f + b_f) omega_fd
 *                                              + sum_j alpha_sj 2 k'(r_j^2) (x~_d - X~_jd) ],  fscale = sqrt(2 amp / F),
 *               k' as in robo_gp_predict_grad: Matern-5/2 -amp (5/6)(1 + t) e^-t with t = sqrt(5 r^2), RBF -amp/2 e^(-r^2/2);
 *               at r = 0 both are finite and the term is 0.
 *   Order.      One wave per descent.  Lane l accumulates the terms of the training rows l, 64 + l, ... and then of the features
 *               l, 64 + l, ... in index order (the value: one FMA per row; the gradient: one per row and coordinate); the 64
 *               lanes' sums meet in a butterfly (xor 32, 16, .., 1).
 *   Descent.    robo_acq_refine_cand's rule applied to -f_s.  Iteration 0 evaluates the start, which always becomes the
 *               current point.  Then n_steps times: g_proj = g with the components that point out of the box at an active
 *               bound set to 0 (x_d <= 0 and g_d > 0, x_d >= 1 and g_d < 0); |g_proj| = sqrt(sum_d g_proj_d^2), summed in
 *               index order, every operation rounded once; |g_proj| = 0 or not finite: the descent is frozen;
 *               y = clip(x - (alpha g_proj) / |g_proj|, 0, 1), each operation rounded once; accept iff f(y) < f(x) (then
 *               x := y, alpha := min(2 alpha, 0.5)), else alpha := alpha / 2.  alpha starts at step0.  A trial whose value is
 *               not finite is not taken and freezes the descent.  Every freeze raises ROBO_FLAG_FROZEN.
 *   Invariance. A descent's whole trajectory depends only on its start point, the snapshot and its own path's weights: not
 *               on P or its slot, on S or the other paths' draws, on the descents it shares a workgroup with, or on which of
 *               the two entry points started it.
 *   Trace.      out_trace ((n_steps + 1) x P x (2 dim + 3), nullable; P = S x n_starts path-major in the fused form): per
 *               iteration and descent the trial point, its value, its gradient, the step length it was made with, and 1 / 0 /
 *               2 / 3 = accepted / rejected / no trial made (frozen earlier or slot unused: the row repeats the current point,
 *               an unused slot carries zeros and a NaN value) / value not finite (not taken; frozen from here on) -- the
 *               layout and meaning of robo_acq_refine_cand's trace.
 * robo_paths_descend runs P descents, descent i on path path_of[i] from x0[i]; out_x, out_value, out_grad (nullable) are the
 * last accepted point, its value and gradient, out_code (nullable) the code of the last iteration.  n_steps = 0 evaluates
 * value and gradient at the given points and nothing else.  A start coordinate outside [0, 1] or not finite, a path_of
 * entry outside 0 .. S - 1, P outside 1 .. ROBO_PATHS_MAX_DESCENTS, n_steps < 0, step0 outside (0, 0.5], a NULL required
 * pointer: ROBO_BAD_ARGUMENT.
 * robo_paths_refine_cand runs the sweep exactly as robo_paths_eval_cand does without values, then selects the starts from
 * what the sweep left on the device -- per path the best row of every group of 64 consecutive candidates (group = row / 64
 * of the whole batch: a pass of the sweep covers a multiple of 128 rows, so the groups do not depend on the chunking).
 * Path s's starts are the n_starts groups' bests with the smallest values, ties by ascending row; a group whose best is NaN
 * (a NaN candidate loses its group) or that has no live row contributes none; fewer eligible groups than n_starts leaves
 * unused slots (row -1 in out_starts (S x n_starts, nullable), never evolved).  Per path the descent with the smallest final
 * value wins, first slot on ties, NaN only if nothing else is there: out_x (S x dim), out_value (S), out_start_index (S: the
 * row of cand the winner started from; -1 and a NaN value when the path has no start).  n_steps = 0 returns the first start
 * -- the sweep's own pick -- with its point and the sweep's value, robo_paths_eval_cand's bits on a batch without NaN.
 * Fed the points of its own out_starts, robo_paths_descend reproduces its trajectories bit for bit.  *out_flags = the
 * sweep's flags | ROBO_FLAG_FROZEN | ROBO_FLAG_NAN (a NaN result).  n_starts outside 1 .. ROBO_PATHS_MAX_STARTS, cand on
 * another context, a NULL required pointer: ROBO_BAD_ARGUMENT; cand's dim is not the paths': ROBO_BAD_SHAPE.
 * Both: dim above 64 (a descent keeps coordinate d in lane d): ROBO_BAD_SHAPE.  All refusals come before anything is
 * launched; one synchronisation per call; the state stays with the paths object.  Event slots 30 and 31 bracket the sweep's
 * passes as above, slots 28 and 29 the descent launch (robo_paths_descend: always; fused: under the condition of 24..27). */
#define ROBO_PATHS_MAX_STARTS 1024      /* per path, as n_starts of robo_acq_refine_cand */
#define ROBO_PATHS_MAX_DESCENTS 65536   /* P */
int32_t robo_paths_descend(robo_paths* p, int32_t P, const int32_t* path_of, const double* x0 /* P x dim */,
                           int32_t n_steps, double step0, double* out_x /* P x dim */, double* out_value /* P */,
                           double* out_grad /* P x dim, nullable */, int32_t* out_code /* P, nullable: last code */,
                           uint32_t* out_flags, double* out_trace /* nullable */);
int32_t robo_paths_refine_cand(robo_paths* p, robo_cand* cand, int32_t n_starts, int32_t n_steps, double step0,
                               double* out_x /* S x dim */, double* out_value /* S */,
                               int64_t* out_start_index /* S: row in cand, -1 when no start */, uint32_t* out_flags,
                               int64_t* out_starts /* S x n_starts, nullable */, double* out_trace /* nullable */);

/* ---- entropy search: replaces InformationGain.innovations/_dh_fun/compute ---------------
 * (robo/acquisition_functions/information_gain.py:87-125,169-203,253-272), batched over candidates.
 * rep: the Nb <= 64 representer points as a candidate batch (same normalised space).  The EP
 * state (log p_min and its derivatives, robo/util/epmgp.py:11-81) is host input:
 *   logP (Nb), lmb (Nb) log proposal values, W (Np <= 512) standard-normal quantiles,
 *   dlogPdMu (Nb,Nb), dlogPdSigma (Nb, Nb(Nb+1)/2) lower-triangle packed, dlogPdMudMu (Nb,Nb,Nb).
 * sn2 = model noise (get_noise()).  out_dh (m,) may be NULL; argmax as robo_acq_eval.         */
int32_t robo_ig_eval_cand(robo_gp* gp, robo_cand* cand, robo_cand* rep, int32_t n_outcomes, double sn2,
                          const double* logP, const double* lmb, const double* W, const double* dlogPdMu,
                          const double* dlogPdSigma, const double* dlogPdMudMu, double* out_dh, double* out_max,
                          int64_t* out_argmax);
/* Information gain PER UNIT COST with its argmax on the device: replaces InformationGainPerUnitCost.compute
 * (robo/acquisition_functions/information_gain_per_unit_cost.py:91-104)
 *     log_cost = self.cost_model.predict(X)[0];  dh = InformationGain.compute(X);  dh / (np.exp(log_cost) + overhead)
 * and the maximiser's argmax over it (robo/maximizers/random_sampling.py:48-50).  cost_gp: the fitted cost model;
 * cost_cand: the SAME m candidates in the cost model's input space (Fabolas: linear basis on the fidelity column where
 * the objective model has (1 - s)^2, robo/fmin/fabolas.py:130-131), a second handle on the same context.
 * out_values (m,) nullable; out_max / out_argmax as robo_acq_eval.                                               */
int32_t robo_ig_eval_per_cost_cand(robo_gp* gp, robo_cand* cand, robo_cand* rep, int32_t n_outcomes, double sn2,
                                   const double* logP, const double* lmb, const double* W, const double* dlogPdMu,
                                   const double* dlogPdSigma, const double* dlogPdMudMu, robo_gp* cost_gp,
                                   robo_cand* cost_cand, double overhead, double* out_values, double* out_max,
                                   int64_t* out_argmax);
/* the same from innovations inputs supplied by any other model: s (m, nb) covariances between each
 * candidate and the representer points, v (m,) predictive variances                              */
int32_t robo_ig_eval_moments(robo_ctx* ctx, int64_t m, int32_t nb, int32_t n_outcomes, double sn2, const double* s,
                             const double* v, const double* logP, const double* lmb, const double* W,
                             const double* dlogPdMu, const double* dlogPdSigma, const double* dlogPdMudMu,
                             double* out_dh);
/* posterior covariances cov(x_c, z_b) (m, nref <= 64), floored at DBL_EPSILON like the reference's
 * predict(full_cov=True) -> predict_variance path (gaussian_process.py:243-246,290-294)            */
int32_t robo_gp_cross_cov(robo_gp* gp, robo_cand* cand, robo_cand* ref, double* out_cov);
/* EP approximation of p_min over nb representer points and its derivatives, for S beliefs N(mu_s, sigma_s) at once:
 * robo/util/epmgp.py joint_min (robo_amd/util/epmgp.py) per belief, one workgroup per (belief, candidate minimiser).
 * mu (S, nb), sigma (S, nb, nb) as predict(full_cov=True) returns them (not required to be exactly symmetric).
 * Outputs per belief in the layouts robo_ig_eval_cand consumes: logP (S, nb); with_derivatives != 0: dlogPdMu
 * (S, nb, nb), dlogPdSigma (S, nb, nb(nb+1)/2) lower-triangle packed, dlogPdMudMu (S, nb, nb, nb) -- NULL allowed when
 * with_derivatives = 0.  out_sweeps (S, nb), nullable: EP sweeps run for each minimiser, -1 where a site's cavity
 * z < -6 killed it (log p floored at -500).  out_status (S): ROBO_OK, ROBO_NOT_POSITIVE_DEFINITE (the closed form's
 * I + R^T Sigma R is singular or not factorable with jitter up to 1e-6; np.linalg.LinAlgError) or ROBO_NUMERIC_ERROR
 * (NaN in the working covariance); a belief's outputs are defined only where its status is ROBO_OK.
 * 1 <= nb <= 64, S >= 1, else ROBO_BAD_ARGUMENT.  Same bits on every call and at every batch position.             */
int32_t robo_ep_joint_min(robo_ctx* ctx, int32_t S, int32_t nb, const double* mu, const double* sigma,
                          int32_t with_derivatives, double* logP, double* dlogPdMu, double* dlogPdSigma,
                          double* dlogPdMudMu, int32_t* out_sweeps, int32_t* out_status);

/* ---- Monte-Carlo entropy search: InformationGainMC (robo/acquisition_functions/information_gain_mc.py, with the
 * intended semantics of DESIGN.md "Monte-Carlo entropy search") and robo/util/mc_part.py joint_pmin with given draws
 * z (nf, nb) row-major: the standard normals, draw f in row f.  The same z is meant for the baseline p_min and every
 * candidate of an update (common random numbers); it is uploaded only when it differs from the last one on the context.
 * Factors: Cholesky of V + j I with j = 0, then 1e-9, x10 while j <= 1e4 (mc_part.joint_pmin's ladder).  A draw's
 * minimum is the first index of the smallest value (np.argmin); p = max(count / nf, 1e-70), not renormalised.
 * Limits: 1 <= nb <= 64, 1 <= n_outcomes <= 512, 1 <= nf <= 65535, else ROBO_BAD_ARGUMENT.  Same bits on every call
 * and at every batch position.                                                                                    */
/* p_min of S beliefs N(mu_s, sigma_s): mu (S, nb), sigma (S, nb, nb) (lower triangle read) -> out_pmin (S, nb),
 * out_jitter (S, nullable) the jitter each factor used, out_status (S): ROBO_OK or ROBO_NOT_POSITIVE_DEFINITE (no factor
 * with jitter up to 1e4; np.linalg.LinAlgError), out_pmin defined only where ROBO_OK.                                */
int32_t robo_pmin_mc(robo_ctx* ctx, int32_t S, int32_t nb, int32_t nf, const double* mu, const double* sigma,
                     const double* z, double* out_pmin, double* out_jitter, int32_t* out_status);
/* information gain of every candidate: s = cov(x, z_b) and v = predictive variance exactly as robo_ig_eval_cand uses
 * them; u = v - sn2, a = s sqrt(v + 1e-10) / u, V_x = Vb - s s^T / u; per outcome p the draws  (Mb + a W_p) + L_x z_f
 * are counted into q[p] (nb); dH = mean_p (H0 - H_p), H = -sum_b p_b (log p_b + lmb_b), H0 from exp(logP).
 * Mb (nb), Vb (nb, nb): the belief at the representer points rep (predict(full_cov=True)); logP (nb) log of its p_min;
 * lmb (nb); W (n_outcomes).  A non-finite dH becomes -DBL_MAX; a candidate whose V_x has no factor gets -DBL_MAX and sets
 * ROBO_FLAG_NOT_FACTORED in out_flags (nullable).  out_dh (m,) nullable; out_max / out_argmax as robo_acq_eval.    */
int32_t robo_igmc_eval_cand(robo_gp* gp, robo_cand* cand, robo_cand* rep, int32_t n_outcomes, int32_t nf, double sn2,
                            const double* Mb, const double* Vb, const double* logP, const double* lmb, const double* W,
                            const double* z, double* out_dh, double* out_max, int64_t* out_argmax, uint32_t* out_flags);
/* the same from innovation inputs supplied by any other model: s (m, nb), v (m).  out_counts (m, n_outcomes, nb),
 * nullable: the raw counts; out_jitter (m), nullable: the jitter each candidate's factor used (the first rung above 1e4
 * where it failed).                                                                                                 */
int32_t robo_igmc_eval_moments(robo_ctx* ctx, int64_t m, int32_t nb, int32_t n_outcomes, int32_t nf, double sn2,
                               const double* s, const double* v, const double* Mb, const double* Vb, const double* logP,
                               const double* lmb, const double* W, const double* z, double* out_dh,
                               int32_t* out_counts, double* out_jitter);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI (SURVEY.md 8b "robo_comm_init + _sharded variants", 8e) -------
 * The reference is single-process; these entry points shard its two independent axes -- the candidate batch of
 * RandomSampling.maximize (robo/maximizers/random_sampling.py:42-50) and the hyper-parameter samples of
 * MarginalizationGPMCMC.compute (robo/acquisition_functions/marginalization.py:115-121) -- and run the one small
 * exchange each of them needs as an RCCL all-gather on the context's stream, device pointers on both sides.  Every
 * rank holds its own replica of the fitted GP(s) (the fit is deterministic).  librccl.so is loaded on first use.
 * COLLECTIVE: every rank of the communicator must make the same call; a rank whose local half fails still takes
 * part in the exchange (as an empty shard) and then returns its error.                                            */
typedef struct robo_comm robo_comm;
#define ROBO_COMM_ID_BYTES 128
/* rank 0 creates the id (ncclGetUniqueId); every rank must receive the same 128 bytes out of band (a file, a TCP
 * store, MPI, torch.distributed.broadcast_object_list ...) before robo_comm_init                                  */
int32_t robo_comm_create_id(void* out_id);
int32_t robo_comm_init(robo_ctx* ctx, int32_t rank, int32_t world, const void* id, robo_comm** out);
int32_t robo_comm_destroy(robo_comm* comm);
int32_t robo_comm_info(robo_comm* comm, int32_t* out_rank, int32_t* out_world);
/* all-gather of `count` host doubles per rank -> recv (world x count), rank-major: the winning point of a
 * device-generated shard, consistency checks, timings -- the few-hundred-byte side channel                         */
int32_t robo_comm_allgather(robo_comm* comm, const double* send, int64_t count, double* recv);
/* candidate shard: robo_acq_eval_cand on this rank's candidates (global index of candidate c = global_offset + c),
 * then the all-gather of the per-rank incumbents (32 B per rank: max, index, flags, status) and np.argmax's tie-break across them on the device.
 * out_max / out_argmax: the GLOBAL maximum and its global index, identical on every rank; out_owner_rank: the rank
 * whose shard holds it; out_flags: OR over all ranks; out_acq (nullable): this rank's m values.                    */
int32_t robo_acq_eval_cand_sharded(robo_comm* comm, robo_gp* gp, int32_t acq_kind, double par, double eta,
                                   robo_cand* cand, int64_t global_offset, double* out_acq, double* out_max,
                                   int64_t* out_argmax, int32_t* out_owner_rank, uint32_t* out_flags);
/* candidate shard of the information gain per unit cost (BASELINE config 4: 65 536 candidates over 8 GPUs):
 * robo_ig_eval_per_cost_cand on this rank's candidates, then the same exchange as robo_acq_eval_cand_sharded.     */
int32_t robo_ig_eval_per_cost_cand_sharded(robo_comm* comm, robo_gp* gp, robo_cand* cand, robo_cand* rep,
                                           int32_t n_outcomes, double sn2, const double* logP, const double* lmb,
                                           const double* W, const double* dlogPdMu, const double* dlogPdSigma,
                                           const double* dlogPdMudMu, robo_gp* cost_gp, robo_cand* cost_cand,
                                           double overhead, int64_t global_offset, double* out_values, double* out_max,
                                           int64_t* out_argmax, int32_t* out_owner_rank);
/* sample shard: this rank's S_local fitted GPs (S_total over all ranks; S_local may be 0) on ALL candidates; the
 * per-rank partial sums are all-gathered (m doubles per rank) and added in rank order on the device, divided by
 * S_total, argmax.  Outputs as robo_acq_eval_marginal_cand, identical on every rank; equal to the single-process
 * sample-order accumulation up to fp64 re-association (partial sums are formed per shard).                         */
int32_t robo_acq_eval_marginal_cand_sharded(robo_comm* comm, robo_gp* const* gps, int32_t S_local, int32_t S_total,
                                            int32_t acq_kind, double par, const double* etas, robo_cand* cand,
                                            double* out_acq, double* out_max, int64_t* out_argmax,
                                            uint32_t* out_flags);

/* ---- multi-GPU, ONE process: G contexts of the calling process, one per device (SURVEY.md 8b "Threading: single process,
 * one context per device") ------------------------------------------------------------------------------------------------
 * The reference is one process with one objective evaluation per iteration (robo/solver/bayesian_optimization.py:156-203).
 * A robo_multi fans the shards of the same two axes as the _sharded entry points above -- candidates
 * (robo/maximizers/random_sampling.py:42-50) and hyper-parameter samples (robo/acquisition_functions/marginalization.py:
 * 115-121, robo/models/gaussian_process_mcmc.py:149-164,235-247) -- over its contexts: one worker thread per device runs the
 * ordinary single-device entry point on that device's context and stream, all devices concurrently, and the G results are
 * reduced -- candidate shards on the host (32 bytes per device arrive through each context's pinned read-back anyway; np.argmax
 * tie-break: NaN maximal, larger value, lower global index), sample shards on the FIRST context's device (peer copies over
 * xGMI, then the rank-ordered sum / mixture kernels of the single-device and _sharded forms: same bits as those).
 * No collective is involved: a failing device cannot hang the others; every call waits for all devices and returns the
 * first failing device's status.  Arrays indexed "[G]" have one entry per context, in the order given to robo_multi_create;
 * every handle of slot g must live on context g.  Several contexts may share a device (tests on a one-GPU box).
 * ROBO_MULTI_THREADS=0 (read at creation) runs the per-device halves one after the other on the caller's thread.        */
typedef struct robo_multi robo_multi;
int32_t robo_multi_create(robo_ctx* const* ctxs, int32_t n_ctx, robo_multi** out);
int32_t robo_multi_destroy(robo_multi* multi);
/* out_devices[G] (nullable): HIP device of every slot; out_threads: worker threads in use (0 = caller's thread)            */
int32_t robo_multi_info(robo_multi* multi, int32_t* out_n, int32_t* out_devices, int32_t* out_threads);
/* the same training data / the same fit on every device (a replica per device; the fit is deterministic: replicas whose
 * status or log-likelihood bits differ are reported as ROBO_RUNTIME_ERROR).  gaussian_process.py:119,122,155          */
int32_t robo_gp_set_data_multi(robo_multi* multi, robo_gp* const* gps, const double* X, const double* y, int32_t n);
int32_t robo_gp_fit_multi(robo_multi* multi, robo_gp* const* gps, const double* theta, double mean_c, double* out_loglik,
                          int32_t* out_fail_col);
/* robo_gp_loglik_batch with the S thetas split contiguously over the devices (the first S % G devices take one more):
 * the walkers of an ensemble half-step (gaussian_process_mcmc.py:114-142,168-202).  gps[G]: one handle per device, each
 * holding the data.                                                                                                       */
int32_t robo_gp_loglik_batch_multi(robo_multi* multi, robo_gp* const* gps, const double* thetas, int32_t S, double mean_c,
                                   double* out_loglik, int32_t* out_status);
/* robo_gp_fit_batch per device: gps[S_total] in device order (S_dev[0] handles of slot 0 first, ...), thetas / outputs in
 * the same order; the FIRST handle of every device's group holds the training data on that device.
 * gaussian_process_mcmc.py:149-164                                                                                         */
int32_t robo_gp_fit_batch_multi(robo_multi* multi, robo_gp* const* gps, const int32_t* S_dev, const double* thetas,
                                double mean_c, double* out_loglik, int32_t* out_status);
/* candidate shard: robo_acq_eval_cand on every device's shard (cands[g] NULL = empty shard), gps[g] = that device's replica;
 * global index of candidate c of slot g = global_offsets[g] + c.  out_acq (nullable): the values of all shards, slot after
 * slot.  out_owner: the slot whose shard holds the maximum; out_flags: OR over the devices.                              */
int32_t robo_acq_eval_cand_multi(robo_multi* multi, robo_gp* const* gps, int32_t acq_kind, double par, double eta,
                                 robo_cand* const* cands, const int64_t* global_offsets, double* out_acq, double* out_max,
                                 int64_t* out_argmax, int32_t* out_owner, uint32_t* out_flags);
/* candidate shard of robo_ig_eval_cand (InformationGain.compute, information_gain.py:87-125,253-272): reps[g] = the
 * representer points on device g, the EP state is the same host input for every device                                     */
int32_t robo_ig_eval_cand_multi(robo_multi* multi, robo_gp* const* gps, robo_cand* const* cands, robo_cand* const* reps,
                                int32_t n_outcomes, double sn2, const double* logP, const double* lmb, const double* W,
                                const double* dlogPdMu, const double* dlogPdSigma, const double* dlogPdMudMu,
                                const int64_t* global_offsets, double* out_dh, double* out_max, int64_t* out_argmax,
                                int32_t* out_owner);
/* candidate shard of robo_ig_eval_per_cost_cand (BASELINE config 4); reps / cost_gps / cost_cands: per-device replicas     */
int32_t robo_ig_eval_per_cost_cand_multi(robo_multi* multi, robo_gp* const* gps, robo_cand* const* cands,
                                         robo_cand* const* reps, int32_t n_outcomes, double sn2, const double* logP,
                                         const double* lmb, const double* W, const double* dlogPdMu,
                                         const double* dlogPdSigma, const double* dlogPdMudMu, robo_gp* const* cost_gps,
                                         robo_cand* const* cost_cands, double overhead, const int64_t* global_offsets,
                                         double* out_values, double* out_max, int64_t* out_argmax, int32_t* out_owner);
/* sample shard of robo_acq_eval_marginal_cand: gps / etas [S_total] in device order, cands[g] = ALL m candidates on device g
 * (NULL allowed where S_dev[g] == 0, g > 0).  Partial sums are formed per device and added in device order: the result equals
 * robo_acq_eval_marginal_cand_sharded with the same shards bit for bit, and the single-device accumulation up to fp64
 * re-association.                                                                                                          */
int32_t robo_acq_eval_marginal_cand_multi(robo_multi* multi, robo_gp* const* gps, const int32_t* S_dev, int32_t acq_kind,
                                          double par, const double* etas, robo_cand* const* cands, double* out_acq,
                                          double* out_max, int64_t* out_argmax, uint32_t* out_flags);
/* sample shard of robo_gp_predict_mixture_cand: the per-sample posteriors are gathered on the first device in sample order
 * and mixed there by the same kernel: identical to the single-device mixture bit for bit.                                  */
int32_t robo_gp_predict_mixture_cand_multi(robo_multi* multi, robo_gp* const* gps, const int32_t* S_dev,
                                           robo_cand* const* cands, double* out_mean, double* out_var);

#ifdef __cplusplus
}
#endif
#endif /* ROBO_HIP_H */
