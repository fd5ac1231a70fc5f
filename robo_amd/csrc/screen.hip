// The acquisition screen: argmax-only sweeps (robo_acq_eval_cand and its sharded / multi-device forms with out_acq == NULL)
// solve only the candidates that can still be the argmax.
//
// The block-row substitution costs O(N^2) per candidate and the caller of an argmax-only sweep sees one winner.  Two facts
// that cost O(N) per candidate decide for almost all of the others that they are not it:
//   * the posterior mean is  mu = k_* . alpha  with  alpha = K^-1 (y - c) = L^-T z,  z = row n of the factor: alpha belongs to
//     the FIT (computed once per fit_gen, by the backward block rows of batch.hip, never from the explicit inverse);
//   * post_kernel forms  v = (k** - q) y_std^2  with q a sum of squares, so  v <= k** y_std^2  holds in floating point too, and
//     v >= DBL_EPSILON by the floor.
// EI, LogEI and LCB (kappa >= 0) increase in sigma and decrease in the mean; PI increases in sigma where its numerator
// eta - mu - xi is negative and decreases where it is positive.  So
//     U_c = acq(mean - delta, prior variance (1 + rho)) (1 + rho)        L_c = acq(mean + delta, floor) (1 - rho)
// bracket the value the sweep would return for candidate c (PI: U = 1 where the numerator can be >= 0, the lower bound at the
// prior variance there).  b = max_c L_c is a value SOME candidate reaches, so a candidate with U_c < b cannot be the argmax
// and cannot tie with it.  The others -- every candidate with a NaN in its screening quantities among them, `U_c < b` is
// false for it -- are gathered in ascending original index and run through the path the unscreened call runs for the whole
// batch (predict_scaled without the explicit inverse, post_kernel, acq_kernel, the argmax).  Block-row results do not depend
// on tile shape or position (tests/test_gpu_parity.py test_small_and_large_candidate_tiles_agree), the gather keeps the index
// order, so (max, argmax, flags) are the unscreened call's bit for bit.
//
// Margins (measured: DESIGN.md "The acquisition screen", tests/test_acq_screen.py):
//   delta = SCREEN_DELTA_REL (|y_mean| + y_std (|mean_c| + sqrt(k_cc) sum_j |alpha_j| sqrt(k_jj)))  -- the scale of the mean's
//           rounding in either route: every product of either sum is bounded by sqrt(k_cc k_jj) |alpha_j|;
//   rho   = SCREEN_RHO relative, on the prior variance and on the value of EI, PI and LogEI (LogEI: of |value| + 1).
// Guard: max L_ii / min L_ii <= SCREEN_DIAG_RATIO_MAX, in the style of winv_factor_ok.
//
// Flags: acq_kernel ORs them over the candidates it sees, here the survivors.  A pruned candidate cannot raise one: NAN needs a
// NaN value, and a NaN in the screening quantities makes a survivor; ZERO_SIGMA needs sqrt(v) == 0 and post_kernel floors v at
// DBL_EPSILON; NEGATIVE_EI needs EI < -DBL_MIN, but z Phi(z) + phi(z) is rounded to a negative number only where both terms
// have underflowed below DBL_MIN (|z| > 37.5 with sigma >= 1.5e-8: the clamp of acq_kernel returns +0 there).
//
// The probe.  Where eta lies below every mean, L_c is the value at the variance floor -- essentially 0 for every candidate --
// and b = max L_c prunes nothing.  When more than the cap survive, the SCREEN_PROBE candidates with the largest U_c (the
// radix selection of refine.hip) are evaluated exactly by the block-row path and b is raised to their best value less rho:
// again a value some candidate reaches.  The probe supplies that bound alone: its values and flags are dropped, the
// survivors (the probed ones among them) are solved afresh.
//
// When more than acq_screen_keep_max percent still survive (eta below every mean: L_c is the value at the variance floor,
// essentially 0 everywhere, and nothing is pruned) the call runs the plain sweep on everything and the factor is not
// screened for the next 1, 2, 4, ... eligible calls: a regime that never prunes pays for the screen a vanishing number of
// times.  A new fit starts afresh.
//
// The dot form.  Two kernels form the bounds.  screen_bounds_kernel accumulates r2 from direct differences on the VALU (32
// of its ~100 fp64 instructions per pair at D = 16); screen_bounds_dot_kernel (Matern-5/2 and RBF, D <= SCREEN_DOT_MAX_D)
// takes  r2 = |a|^2 + |b|^2 - 2 a.b  from v_mfma_f64_16x16x4_f64, which is idle in the first: training rows are the A operand
// -2 b, candidates the B operand a, both CENTRED  (a = x_c - ctr, b = x_j - ctr, ctr the mid-range of the scaled training
// rows per dimension: r2 does not move, the norms shrink to the data's half-extent), the contraction padded with zeros to
// K = 4 KS >= D.  The norms cost no instruction of their own: |b|^2 is the accumulator's initial value (the C operand), |a|^2
// the addend of the FMA that scales r2 for the covariance function anyway.  (Two extra K columns [|b|^2, 1] x [1, |a|^2]
// were built first: 5 k-steps instead of 4 at D = 16 and 5 instead of 2 at D = 8, same VALU count, 0.90 against
// 0.88 ms for the headline step.)  The rows, the norms, amp alpha and the scalars below are laid out once per fit_gen
// (alpha_ensure), never per call.
//   Error of that r2.  With u = 2^-53, eps = 2 u:
//     centring   a_d, b_d carry a relative u each, so (a_d - b_d)^2 moves by <= 2 u (|a_d| + |b_d|)^2 <= 2 eps (a_d^2 + b_d^2):
//                summed, 2 eps (|a|^2 + |b|^2);
//     norms      |a|^2, |b|^2 by D FMAs: (D + 1) u each, <= (D + 1) eps (|a|^2 + |b|^2) / 2;
//     product    K terms accumulated by the matrix pipe, one rounding per step; the terms' magnitudes sum to
//                |a|^2 + |b|^2 + 2 sum_d |a_d b_d| <= 2 (|a|^2 + |b|^2):  K u 2 (|a|^2 + |b|^2) = K eps (|a|^2 + |b|^2);
//                the factor -2 of the staged rows is exact;
//     clamp      r2 >= 0 in exact arithmetic, so max(r2, SD_R2_MIN) moves the computed value towards the true one (or by 1e-290).
//     finish     |a|^2 enters as fma(5, acc, 5 |a|^2) (RBF: -1/2): one rounding of the product 5 |a|^2 and one of the sum,
//                <= 2 u (|a|^2 + |b|^2) in r2;
//   Together < (K + 6) 2 eps (|a|^2 + |b|^2) / 2; the kernel uses (K + 6) 2 eps (|a|^2 + max_j |b_j|^2), twice that, as the
//   bound |dr2| (gram_tile.h has the same analysis for the fit's tile, with (D + 3)).
//   Effect on the mean.  |dk/dr2| <= amp c_KIND with c = 5/6 (Matern-5/2: dk/dr2 = -(5/6)(1 + s) e^-s, s = sqrt(5 r2), largest
//   at s = 0) and c = 1/2 (RBF), so  |d mu~| <= y_std amp c_KIND |dr2| sum_j |alpha_j|.  Candidate c's delta gains
//       SCREEN_DOT_SAFETY y_std amp c_KIND (K + 6) 2 eps (|x_c - ctr|^2 + max_j |x_j - ctr|^2) sum_j |alpha_j|
//   evaluated in the kernel from its own centred norm: a candidate far outside the data box loosens its own bound only (a NaN
//   or infinite coordinate makes the term, hence both bounds, NaN or vacuous: a survivor).  The sum's own rounding (four
//   lane groups of 4 rows per tile, added in a fixed order) and amp folded into alpha are of the size SCREEN_DELTA_REL
//   covers already.
//   Selection (launch_screen_bounds).  The dot kernel runs where the kind and D permit, acq_screen_dot allows (-1 rule, 0
//   never, 1 always) and, under the rule, gram_needs_direct's figure with centred extents,
//       (D + 3) 2 eps sum_d max_j (x_jd - ctr_d)^2        (scaled rows; computed on the device with the centre),
//   is at most SCREEN_DOT_BOUND = GRAM_DIRECT_BOUND = 1e-12.  Measured (tests/test_acq_screen_dot.py): at that bound the
//   largest |mu~ - mu_sweep| stays below 1e-4 of the delta the kernel applies; the headline theta gives 8.4e-15.  The direct
//   kernel keeps Fabolas, D above the limit and every theta beyond the bound (ln m = -10 at the prior's edge).
//
// The lean finish (screen_dot_finish_lean; Matern-5/2 and RBF, the dot kernel only).  The finish above evaluates sqrt and exp
// to the last bit (35 fp64 VALU instructions per pair, 26 of them sqrt + exp) for a mean whose margin is 1e-11 sum |alpha|.
// The lean finish evaluates k~ with  |k~ - k| <= SD_LEAN_EPS amp,  SD_LEAN_EPS = 8e-13  (27 instructions), and candidate c's
// delta gains   SCREEN_LEAN_SAFETY SD_LEAN_EPS |y_std| sum_j |amp alpha_j|,   SCREEN_LEAN_SAFETY = 1e4: with a true bound
// the mean moves by at most 1e-4 of the delta applied, the ratio tests/test_acq_screen_dot.py asserts.
//   Error of that k~, in units of amp, u = 2^-53.  Matern-5/2: k = q e^-s, q = 1 + s + t / 3, s = sqrt(t), t = 5 r2; RBF: q = 1,
//   x = -r2 / 2.  The error of r2 itself is the dot form's term above; here t (x) is taken as given.
//     seed       y0 = rsq(t) = (1 + d) / sqrt(t).  e = 1 - t y0^2 = -2 d - d^2, and  y0 (1 + e / 2 + 3 e^2 / 8)  is 1 / sqrt(t)
//                up to (5 / 16) |e|^3 (1 + |e|): the 0.375 e term is KEPT, only the residual step  s += (t - s^2) y / 2  is
//                dropped.  The proof needs |d| <= 2^-18 of the seed.  No figure of the ISA manual is cited for that: the form is
//                chosen so as not to depend on one (kern_math.h takes v_rsq_f64 as ~2^-23, 32 times better, and the MI355X
//                twin of the finish test reproduces the interpreter's error to four digits): then |e| <= 7.7e-6 and the truncation is 1.5e-16.  Roundings: t y0, e (absolute u: it enters
//                times y0 / 2), y0 e, the inner and the outer FMA, s = t y:  s~ = s (1 + rho), |rho| <= 4 u + 1.5e-16 < 6e-16.
//     its effect q is formed from the same s~, so  k~(s~) = (1 + s~ + t / 3) e^-s~  and  |d k~ / d ln s| = s^2 (1 + s / 3) e^-s
//                <= 0.942 (at s = sqrt 6):  0.942 rho < 5.7e-16.
//     q          1 + s~ and the FMA: 2 u q; the constant 1/3: u t / 3 <= u q.  With k <= 1:  3 u = 3.4e-16.
//     reduction  n = rint(x log2 e); r = fma(n, -L, x) with ONE constant
//                L = 0x1.62e42fefa39efp-1, |L - ln 2| = 2.32e-17, so r is off by |n| 2.32e-17 + u |r|: relative in e^x.
//                |n| <= |x| / ln 2 + 1/2 and  k |x| <= max_s s q e^-s = 1.18:  < 1.18 / ln 2 x 2.32e-17 + u < 2e-16 in k.
//                |r| <= ln 2 / 2 (1 + 2^-40): the rounding of x log2 e moves the tie by |x| u <= 8e-14.
//     polynomial degree 8, Remez for the relative error of e^r on |r| <= (ln 2 / 2)(1 + 1e-3), coefficients rounded to
//                double, evaluated with fp64 FMA Horner steps on 2e6 points against long double: 7.8153e-13 (the fit's
//                levelled error 7.8142e-13; tools/exp_lean_coeffs.py prints both, and 1.4e-14 for degree 9, 5.4e-11 for 7).
//                That figure is SAMPLED, not a maximum over the interval: neighbouring points lie h = 3.5e-7 apart, and the
//                error's derivative is (p' - p) e^-r with |p' - p| <= 6e-9 (the degree-8 truncation term r^8 / 8!, 5.2e-9 at
//                the edge, plus the fit's 1e-12), so between two points it moves by at most 2.1e-15: <= 7.84e-13.
//                Relative in e^x, and q e^x <= 1.
//     2^n        v_ldexp_f64, as in the full finish: exact down to the subnormals (there off by <= 2^-1075) and 0 below them by
//                itself, so a far candidate gives k~ = 0 or a subnormal times q, never a large number; no clamp of x is needed
//                (with |x| > 745 both k and k~ are below 1e-300 whatever r is).  The lower clamp of t (x) is the full finish's.
//                (t = inf or NaN: k~ is NaN, and so is the candidate's norm term of delta: a survivor, as above.)
//     product    q times p 2^n: u.
//   Sum: 7.84e-13 + 5.7e-16 + 3.4e-16 + 2e-16 + 1.2e-16 < 7.86e-13 < SD_LEAN_EPS.  Measured (tests/test_acq_screen_lean.py,
//   N = 1 so that the mean is one product): 7.81e-13 (Matern-5/2), 7.28e-13 (RBF), interpreter and MI355X alike.
//   The rule (screen_lean_wanted).  acq_screen_lean: -1 the rule, 0 never, 1 wherever the dot kernel runs.  Under the rule the
//   lean finish runs where its term is at most SCREEN_LEAN_MAX = 1e-2 of the prior standard deviation |y_std| sqrt(amp),
//       SCREEN_LEAN_SAFETY SD_LEAN_EPS sqrt(amp) sum_j |alpha_j| <= 1e-2        (sum_j |alpha_j| <= 1.25e6 at amp = 1)
//   -- U_c falls by at most delta while the prior variance it is taken at is loose by orders more.  The headline's fit gives
//   2.7e-3, config 2's 1.4e-3; a nearly singular K (tiny noise, long length scales) takes the full finish, whose kernel and
//   delta are the previous ones bit for bit.  sum_j |alpha_j| reaches the host in alpha_ensure's one copy per fit_gen.
//
// The single-precision first stage (screen_dot_finish_single; acq_sweep_best's cascade).  The chained solve costs the same for
// 1 and for 128 survivors, and the survivor count stays below a dozen while delta is a few tenths of the prior standard
// deviation (NOTES.md "A single-precision first stage"), so an argmax-only call first forms its bounds from a covariance
// good to  |k~ - k| <= SD_SINGLE_EPS amp,  SD_SINGLE_EPS = 6.3e-7:  the fp64 MFMA distance, the centred norms, alpha, the four
// fp64 accumulators and the reduction as in the other finishes, but t (x) rounded to float and k~ from v_sqrt_f32, v_exp_f32
// and five more fp32 instructions.  Candidate c's delta gains
//     SCREEN_SINGLE_SAFETY SD_SINGLE_EPS |y_std| sum_j |amp alpha_j|,     SCREEN_SINGLE_SAFETY = 1.5   (together 9.45e-7).
//   Error of that k~, in units of amp, v = 2^-24 (the unit roundoff of float).  k = q e^-s, q = 1 + s + t / 3, s = sqrt(t) as
//   above; t (x) in fp64 is taken as given, and the fp64 steps in front of the conversion are the lean finish's.
//   Hardware figures ASSUMED: v_sqrt_f32 and v_exp_f32 return their result within 1 ulp (relative 2 v) of the exact function of
//   the float they are given (the CDNA ISA manual's accuracy table); the conversions and v_add / v_mul / v_fma_f32 round to
//   nearest.  tests/test_acq_screen_single.py measures the whole finish on every float of the binade [4, 8) of t.
//     rounding t  t~ = t (1 + d), |d| <= v:  s moves by v / 2 relative, and |dk / d ln s| = s^2 (1 + s) e^-s / 3 <= 0.60 (at
//                s = 1 + sqrt 3; q is formed from t~ and s~ = sqrt(t~) consistently); taken at the lean finish's 0.942:  0.47 v.
//     root        s~ = sqrt(t~) (1 + 2 v'):  0.942 x 2 v = 1.88 v.
//     q           1 + s~ one rounding (<= v q), the FMA one (v q), the constant 1/3 as a float is off by 2.98e-8 = 0.5 v
//                relative (v t / 6 <= 0.5 v q):  2.5 v q, and q e^-s <= 1:  2.5 v.
//     exponent    the argument of 2^x is ONE product  s~ x (-log2 e as a float):  the constant is off by 1.33e-8 = 0.224 v
//                relative, the product rounds once (v):  1.224 v |x| in x, i.e. 1.224 v s relative in e^-s, and
//                k s <= max_s s q e^-s = 1.18:  1.45 v.  (A residual-corrected argument -- a second FMA with the constant's
//                low part -- would take 0.26 v of that; the budget does not need it.)
//     2^x         1 ulp: 2 v relative, k <= 1:  2 v.  Below 2^-126 the instruction returns 0 (no denormals): off by < 1.2e-38.
//     product     q~ e~ one rounding:  v.  The conversion to double is exact, the FMA with alpha is the other finishes'.
//   Sum: (0.47 + 1.88 + 2.5 + 1.45 + 2 + 1) v = 9.3 v; second-order terms (products of two of the above) < 0.1 v; the lean
//   fp64 steps in front 1e-15.  9.4 v = 5.6e-7 < SD_SINGLE_EPS = 10.5 v = 6.3e-7.  RBF (q = 1, x = -r2 / 2): rounding x (v),
//   the product with log2 e (1.224 v), each times |x| e^x <= 1 / e, and 2 v of 2^x:  2.9 v.
//   No select.  The lower clamp of t (x) stays, in fp64; t below the floats' range becomes 0 and gives s = 0, k~ = 1 (true k
//   within 1e-38 of it).  A far candidate: s and q stay finite floats up to t = 3.4e38, 2^x is 0 from x = -150 on, so k~ is 0,
//   never a large number.  t beyond the floats' range (r2 > 6.8e37) or a NaN / infinite coordinate gives k~ = NaN (inf x 0):
//   the mean and both bounds are NaN, `U_c < b` is false, a survivor -- and the NaN / infinite coordinate makes the norm term
//   of delta NaN whatever k~ is, as above.
//   The rule (screen_single_wanted).  acq_screen_single: -1 the rule, 0 never, 1 wherever the lean finish runs, 2 as 1 and
//   robo_acq_screen_bounds returns the FIRST STAGE's bounds instead of the fp64 ones (tests; under every other value it
//   returns the fp64 bounds, bit for bit what it returned before).  Under the rule the first stage runs where the lean finish
//   is selected, its term is at most SCREEN_SINGLE_MAX = 0.5 of the prior standard deviation,
//       SCREEN_SINGLE_SAFETY SD_SINGLE_EPS sqrt(amp) sum_j |alpha_j| <= 0.5            (sum_j |alpha_j| <= 5.3e5 at amp = 1)
//   (the headline's fit: 0.32, config 2's: 0.16), and the factor is not in the first stage's own pause.
//   The cascade (acq_sweep_best).  First stage admitted: scale_inputs, the bounds kernel with the single finish, the count, the
//   one synchronisation.  With 1 <= kept <= min(NB, cap) the call goes on from the gather exactly as after the fp64 pass -- the
//   same launches, no further synchronisation; every survivor of the fp64 bounds is among the first stage's (its U_c is
//   larger, its b smaller), so (max, argmax, flags) are the same bits.  Otherwise the fp64 path runs on the whole batch from
//   launch_screen_bounds, unchanged (count, probe, cap, fall-back, screen_skip), and the factor's first stage pauses for
//   1, 2, 4, ... eligible calls (reset by a new fit, back to 1 after a success): a regime the first stage cannot decide pays
//   its kernel a vanishing number of times.
//
// The integer form (screen_bounds_dot_int_kernel; the first stage only, D <= 16).  The first stage rounds r2 to a float, so
// the fp64 matrix pipe's only job there is to avoid the cancellation in |a|^2 + |b|^2 - 2 a.b; v_mfma_i32_16x16x64_i8
// accumulates in int32 with no rounding at all and holds the pipe 16 cycles against 64 (measured: NOTES.md).
//   Grid (per fit_gen, screen_dot_prep_kernel).  H = max_jd |x_jd - ctr_d| over the centred scaled training rows;
//   h = 2 H / SD_INT_GRID, SD_INT_GRID = 8 355 000: +-2 H (candidates are drawn from the box of the data, whose centre is not
//   the rows' mid-range) lies inside +-SD_INT_AMAX = 127 (2^16 + 2^8 + 1), the largest integer three balanced digits hold.
//   A = rint(a / h) = A0 2^16 + A1 2^8 + A2, digits in [-128, 127] (the sign-extended low byte of what is left).  Rows with no
//   extent (H = 0: one row) have no grid of their own: the rule refuses, key 1 takes H = 1/2.
//   Operands.  Lane group g = l >> 4 of the A operand holds digit g of the row in dimensions 0 .. 15 (group 3: zeros), once
//   per fit (screen_int_pack_kernel): ONE 16-byte LDS read per lane and tile serves four products whose B operands, built
//   once per candidate, are [B0 0 0 0], [B1 B0 0 0], [B2 B1 B0 0], [0 B2 B1 0]:
//       S0 = sum A0 B0 (2^32)   S1 = sum A0 B1 + A1 B0 (2^24)   S2 = sum A0 B2 + A1 B1 + A2 B0 (2^16)   S3 = sum A1 B2 + A2 B1 (2^8)
//   in units of h^2; |S2| <= 3 x 16 x 2^14, no level leaves int32.  S4 = sum A2 B2 is dropped.
//   Combine.  T0 = 256 S0 + S1, T1 = 256 S2 + S3 (int32), P = 2^16 T0 + T1, u = (|A|^2 + |B|^2 + SD_INT_OFF) - 512 P in fp64:
//   all integers below 2^53, so u = |A - B|^2 + 2 S4 + SD_INT_OFF EXACTLY.  SD_INT_OFF = 2^19 >= 2 |S4| (D <= 16, digits
//   <= 2^7) is added to |B|^2 once per candidate: u >= 0 always, no clamp; it and S4 together move u by [0, 2^20].
//   t = 5 h^2 u (RBF: x = -h^2 u / 2): one fp64 rounding, then screen_single_cov, the single finish's float part unchanged.
//   Per pair 17 instructions (the fp64-MFMA form: 11): 2 v_lshl_add_u32, 2 v_cvt_f64_i32, v_fmac_f64, v_add_f64, v_fmac_f64,
//   v_mul_f64, and the 9 from v_cvt_f32_f64 on.
//   Error of that k~, in units of amp, next to SD_SINGLE_EPS (which covers everything from the float conversion on).
//     grid       a = h A + e_a, |e_a,d| <= h / 2 (the rounding of the centring, u |a_d|, and of a x fl(1 / h), 2^-29 h, are
//                inside the slack of the constants below); likewise b.  With r~ = h |A - B|:  |r~ - r| <= |e_a - e_b|_2 <=
//                sqrt(D) h (triangle inequality), and k is Lipschitz in r:  Matern-5/2  |dk/dr| = (sqrt 5 / 3) s (1 + s) e^-s
//                <= 0.6261 (at s = (1 + sqrt 5) / 2);  RBF  |dk/dr| = r e^(-r^2 / 2) <= e^(-1/2) = 0.6066.
//                |dk| <= c1 sqrt(D) h,  c1 = 0.63 (Matern-5/2), 0.61 (RBF):  1.5e-7 at the headline (H = 0.25, h = 6.0e-8).
//     S4, offset r2 moves by at most 2^20 h^2 and |dk/dr2| <= c2 = 5/6 (1/2):  c2 2^20 h^2 = 3e-9 at the headline.
//     product    5 h^2 as a double and t: 3 u relative in t, |dk/d ln t| <= 0.47:  2e-16.
//   SD_INT eps = c1 sqrt(D) h + c2 2^20 h^2 is per fit (st[SD_INT + 2]); candidate c's delta gains, in place of the fp64 dot
//   form's r2 term (which no longer applies),
//       SCREEN_SINGLE_SAFETY (SD_SINGLE_EPS + eps_c) |y_std| sum_j |amp alpha_j|
//   with eps_c = that figure;  = 1 for a FAR candidate -- a finite coordinate beyond +-SD_INT_AMAX h is clamped to it, and k~,
//   k both lie in [0, 1]: a finite, rigorous, vacuous bound (U_c is then huge: a survivor in practice);  = NaN for a
//   non-finite coordinate (the integer conversion would not propagate it): both bounds NaN, a survivor.  More than a tile of
//   either kind makes the first stage miss and pause through the cascade's own path.
//   The rule (screen_int_wanted).  acq_screen_int: -1 the rule, 0 never, 1 wherever the first stage runs and D <= 16.  Under
//   the rule: 8 < D <= 16 (four k-steps of the fp64 form; at D = 8 the integer form measured no faster), the rows have an
//   extent, and the stage's WHOLE term stays within SCREEN_SINGLE_MAX:
//       SCREEN_SINGLE_SAFETY (SD_SINGLE_EPS + eps) sqrt(amp) sum_j |alpha_j| <= 0.5               (the headline's fit: 0.39)
//   Otherwise the fp64-MFMA first stage runs under its own rule.  robo_cand_last_screen_form reports the form;
//   bounds_kernel() keeps naming the dot kernel's family.  Measured (tests/test_acq_screen_int.py): on the grid the error is the
//   float finish's alone (1.3e-7), off it 1.0e-7 against 7.8e-7 allowed at D = 16.
#include <cmath>

#include "api_internal.h"
#include "kern_math.h"

namespace robo {

constexpr double SCREEN_DELTA_REL = 1e-11;
constexpr double SCREEN_RHO = 1e-5;
constexpr double SCREEN_DIAG_RATIO_MAX = 1e4;
constexpr int SCREEN_PROBE = NB;     // candidates of the probe: one tile
constexpr int SCREEN_DOT_MAX_D = 32;          // the dot kernel's k-loop: KS = 1, 2, 4 (D <= 16, the tuned case) or 8 k-steps of 4
constexpr double SCREEN_DOT_SAFETY = 4.0;
constexpr double SCREEN_DOT_BOUND = GRAM_DIRECT_BOUND;     // worst-case r2 error a theta may carry into the dot kernel (measured: header)

constexpr int SC_CAND = 64;          // candidates per workgroup of the bounds pass (one per lane; the 4 waves split the rows)
constexpr int SC_ROWS = 32;          // training rows per wave and tile
constexpr int SC_LD = NB + 2;

// ---- alpha's scale: sum_j |alpha_j| sqrt(k_jj) -> out[0] ---------------------------------------------------------------
__global__ __launch_bounds__(256) void screen_alpha_norm_kernel(const double* __restrict__ alpha, const double* __restrict__ Xs,
                                                                CovParams cp, int n, double* __restrict__ out) {
    __shared__ double sh[256];
    double a = 0.0;
    for (int j = threadIdx.x; j < n; j += 256)
        a += fabs(alpha[j]) * sqrt(fabs(cov_self(cp, Xs[(size_t)j * cp.dim + cp.dim - 1])));
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sh[0];
}

// x moved outwards by rho (|x| + abs_term); infinities and NaN stay what they are
__device__ __forceinline__ double screen_widen(double x, double sign, double abs_term) {
    return isfinite(x) ? x + sign * SCREEN_RHO * (fabs(x) + abs_term) : x;
}

// the two bounds of one candidate from its transformed mean m (+- delta), the transformed prior variance and the floor
__device__ __forceinline__ void screen_bounds(int kind, double par, double eta, double m, double delta, double v_prior,
                                              double& up, double& lo) {
    const double eps = 2.220446049250313e-16;
    double v_hi = v_prior < eps ? eps : v_prior;     // the floor of post_kernel; NaN propagates
    v_hi = v_hi * (1.0 + SCREEN_RHO);
    const double v_lo = eps;
    const double m_lo = m - delta, m_hi = m + delta;
    if (kind == ROBO_ACQ_EI) {
        up = acq_ei(m_lo, v_hi, eta, par);
        lo = acq_ei(m_hi, v_lo, eta, par);
        if (up < 0.0 && up > -2.2250738585072014e-308) up = 0.0;     // as acq_kernel
        if (lo < 0.0 && lo > -2.2250738585072014e-308) lo = 0.0;
        up = screen_widen(up, 1.0, 0.0);
        lo = screen_widen(lo, -1.0, 0.0);
    } else if (kind == ROBO_ACQ_LOG_EI) {
        up = screen_widen(acq_log_ei(m_lo, v_hi, eta, par), 1.0, 1.0);
        lo = screen_widen(acq_log_ei(m_hi, v_lo, eta, par), -1.0, 1.0);
    } else if (kind == ROBO_ACQ_PI) {
        // Phi(num / sigma) falls in sigma where num > 0: no bound from the prior variance above, the lower one from it
        up = (eta - m_lo - par >= 0.0) ? 1.0 : screen_widen(acq_pi(m_lo, v_hi, eta, par), 1.0, 0.0);
        lo = screen_widen(acq_pi(m_hi, (eta - m_hi - par >= 0.0) ? v_hi : v_lo, eta, par), -1.0, 0.0);
    } else {
        // a plain sum: its rounding is eps (|m| + kappa sigma), far inside delta (|m| <= the scale delta is taken from)
        up = acq_lcb(m_lo, v_hi, par);
        lo = acq_lcb(m_hi, v_lo, par);
    }
}

// ---- b = max_c L_c, formed inside both bounds kernels (NaN ignored; -inf when there is none) -----------------------------------
// One maximum per workgroup, one atomicMax per workgroup on an order-preserving 64-bit key of the double; the slot is set to the
// key of -inf by the scale_inputs launch that precedes the pass.  A maximum does not depend on order: b keeps its bits.
__device__ __forceinline__ unsigned long long screen_key(double x) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double screen_unkey(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}
constexpr unsigned long long SCREEN_KEY_NONE = 0x000FFFFFFFFFFFFFull;      // screen_key(-inf)

__device__ __forceinline__ double screen_block_max(double x, double* sh) {
    for (int o = 32; o > 0; o >>= 1) {
        const double y = __shfl_xor(x, o);
        x = y > x ? y : x;
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
    __syncthreads();
    double r = sh[0];
    for (int w = 1; w < 4; ++w) r = sh[w] > r ? sh[w] : r;
    return r;
}

// ---- the bounds pass -------------------------------------------------------------------------------------------------------
// SIBLING of batch_cond_kernel (batch.hip): the same staging, SMALLD split and pair loop -- change the two together.  A
// workgroup owns 64 candidates, one per lane; its four waves split every
// tile of 128 training points (32 rows each, staged as [dimension][row]: a broadcast read).  Per pair the covariance is
// accumulated dimension by dimension with direct differences, as the cross-gram generators of predict.hip do, and
// multiplied into the lane's running k_* . alpha.  No V, no workspace.
template <int KIND, bool SMALLD>
__global__ __launch_bounds__(256) void screen_bounds_kernel(const double* __restrict__ Xcs, const double* __restrict__ Xs,
                                                            const double* __restrict__ alpha,
                                                            const double* __restrict__ alpha_norm, CovParams cp, int n,
                                                            long long m, double mean_c, double y_mean, double y_std,
                                                            int acq_kind, double par, double eta, double* __restrict__ up,
                                                            double* __restrict__ lo, unsigned long long* __restrict__ bkey) {
    __shared__ double sX[16 * SC_LD];
    __shared__ double sA[NB];
    __shared__ double sP[4][SC_CAND];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, D = cp.dim;
    const long long i = (long long)blockIdx.x * SC_CAND + lane;
    const bool live = i < m;
    const long long ii = live ? i : 0;
    double xc[16];
    if (SMALLD) {
#pragma unroll
        for (int d = 0; d < 16; ++d) xc[d] = d < D ? Xcs[ii * D + d] : 0.0;
    }
    const int nbk = (n + NB - 1) / NB;
    double dot = 0.0;
    for (int tile = 0; tile < nbk; ++tile) {
        double acc[SC_ROWS], uu[SC_ROWS];
#pragma unroll
        for (int r = 0; r < SC_ROWS; ++r) cov_init<double, KIND>(cp, acc[r], uu[r]);
        for (int d0 = 0; d0 < D; d0 += 16) {
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int idx = tid + e * 256, row = idx >> 4, d = idx & 15;
                const int rg = tile * NB + row;
                sX[d * SC_LD + row] = (d0 + d < D && rg < n) ? Xs[(size_t)rg * D + d0 + d] : 0.0;
            }
            if (d0 == 0 && tid < NB) sA[tid] = tile * NB + tid < n ? alpha[tile * NB + tid] : 0.0;
            __syncthreads();
            const int dn = D - d0 < 16 ? D - d0 : 16;
            const double* sx = sX + wave * SC_ROWS;
            if (SMALLD) {
#pragma unroll
                for (int d = 0; d < 16; ++d) {
                    if (d < dn) {
#pragma unroll
                        for (int r = 0; r < SC_ROWS; ++r)
                            cov_step<double, KIND>(cp, d, xc[d], sx[d * SC_LD + r], acc[r], uu[r]);
                    }
                }
            } else {
                for (int d = 0; d < dn; ++d) {
                    const double xi = Xcs[ii * D + d0 + d];
#pragma unroll
                    for (int r = 0; r < SC_ROWS; ++r)
                        cov_step<double, KIND>(cp, d0 + d, xi, sx[d * SC_LD + r], acc[r], uu[r]);
                }
            }
        }
        // rows >= n (the augmented row, the padding) take no part
#pragma unroll
        for (int r = 0; r < SC_ROWS; ++r) {
            const double kv = cov_finish<double, KIND>(cp, acc[r], uu[r]);
            if (tile * NB + wave * SC_ROWS + r < n) dot = fma(kv, sA[wave * SC_ROWS + r], dot);
        }
    }
    sP[wave][lane] = dot;
    __syncthreads();
    if (wave != 0) return;
    double lmax = -__builtin_huge_val();
    if (live) {
        const double mu = (sP[0][lane] + sP[1][lane]) + (sP[2][lane] + sP[3][lane]);
        const double kself = cov_self(cp, Xcs[i * D + D - 1]);
        double mt = mu + mean_c;
        mt = mt * y_std + y_mean;
        const double v_prior = kself * (y_std * y_std);
        const double delta = SCREEN_DELTA_REL * (fabs(y_mean) + fabs(y_std) * (fabs(mean_c) + sqrt(fabs(kself)) * alpha_norm[0]));
        double u, l;
        screen_bounds(acq_kind, par, eta, mt, delta, v_prior, u, l);
        up[i] = u;
        lo[i] = l;
        if (!isnan(l)) lmax = l;
    }
    // the workgroup's 64 candidates live in wave 0
    for (int o = 32; o > 0; o >>= 1) {
        const double y = __shfl_xor(lmax, o);
        lmax = y > lmax ? y : lmax;
    }
    if (lane == 0) atomicMax(bkey, screen_key(lmax));
}

// ---- the bounds pass, dot form ------------------------------------------------------------------------------------------------
// The same bounds from  r2 = |a|^2 + |b|^2 - 2 a.b  on the matrix pipe (header: "The dot form").  Once per fit_gen
// screen_dot_prep_kernel finds the centre and the three scalars of the delta term, and screen_dot_pack_kernel lays the
// centred training rows and amp alpha out in the order the bounds kernel consumes them:
//     rows   [tile of 16 rows][k-step kk][lane l]  =  A[i = l & 15][k = 4 kk + (l >> 4)]  of the row  [-2 b_0 .. -2 b_{D-1}, 0 ..]
//     alpha  [stage of 128 rows][0][tile of 16 rows][g = l >> 4][r]  =  amp alpha[16 tile + g + 4 r]   (the rows of lane l's D registers)
//     norms  [stage of 128 rows][1][tile of 16 rows][g = l >> 4][r]  =  |b|^2 of the same rows: the accumulator's initial value
// with zeros for rows >= n (they take no part: the FMA adds k * 0).
template <int N>
__device__ __forceinline__ double screen_block_reduce(double x, double* sh, int op) {     // op 0 sum, 1 max; N threads
    __syncthreads();
    sh[threadIdx.x] = x;
    __syncthreads();
    for (int o = N / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const double y = sh[threadIdx.x + o];
            sh[threadIdx.x] = op == 0 ? sh[threadIdx.x] + y : (y > sh[threadIdx.x] ? y : sh[threadIdx.x]);
        }
        __syncthreads();
    }
    return sh[0];
}

// st[1] = sum_j |alpha_j|, st[2] = max_j |x_j - ctr|^2, st[3] = sum_d max_j (x_jd - ctr_d)^2, st[SD_CTR + d] = ctr_d (mid-range)
// and the integer form's grid (header: "The integer form"): st[SD_INT] = h, + 1: 1 / h, + 2: its covariance error in units of
// amp, + 3: H = max_jd |x_jd - ctr_d| (0: the rows have no extent and the grid is the fall-back's, which only key 1 takes)
constexpr int SD_CTR = 4;
constexpr int SD_INT = SD_CTR + SCREEN_DOT_MAX_D;
constexpr int SD_STATS = SD_INT + 4;
constexpr int SD_INT_MAX_D = 16;                 // one lane group of 16 bytes per digit
constexpr double SD_INT_AMAX = 8355711.0;        // 127 (2^16 + 2^8 + 1): the largest |A| three balanced digits hold
constexpr double SD_INT_GRID = 8355000.0;        // 2 H / h: +-2 H lies inside +-AMAX with room for the roundings of the centring
constexpr double SD_INT_OFF = 1048576.0 / 2;     // 2^19 >= 2 |S4| at D <= 16: added to |B|^2, keeps the integer r2 >= 0 without S4
constexpr double SD_INT_H0 = 0.5;                // H of the fall-back grid
__global__ __launch_bounds__(256) void screen_dot_prep_kernel(const double* __restrict__ alpha, const double* __restrict__ Xs,
                                                              int D, int n, int matern, double* __restrict__ st) {
    __shared__ double sh[256];
    __shared__ double sc[SCREEN_DOT_MAX_D];
    const double inf = __builtin_huge_val();
    double ext = 0.0, H = 0.0;
    for (int d = 0; d < D; ++d) {
        double hi = -inf, nlo = -inf;
        for (int j = threadIdx.x; j < n; j += 256) {
            const double x = Xs[(size_t)j * D + d];
            hi = x > hi ? x : hi;
            nlo = -x > nlo ? -x : nlo;
        }
        hi = screen_block_reduce<256>(hi, sh, 1);
        nlo = screen_block_reduce<256>(nlo, sh, 1);
        const double c = 0.5 * (hi - nlo), h = hi - c, l = c + nlo;
        ext += fmax(h * h, l * l);
        H = fmax(H, fmax(h, l));
        if (threadIdx.x == 0) sc[d] = c;
    }
    __syncthreads();
    double a = 0.0, r = 0.0;
    for (int j = threadIdx.x; j < n; j += 256) {
        a += fabs(alpha[j]);
        double s = 0.0;
        for (int d = 0; d < D; ++d) {
            const double b = Xs[(size_t)j * D + d] - sc[d];
            s = fma(b, b, s);
        }
        r = s > r ? s : r;
    }
    a = screen_block_reduce<256>(a, sh, 0);
    r = screen_block_reduce<256>(r, sh, 1);
    if (threadIdx.x == 0) {
        st[1] = a;
        st[2] = r;
        st[3] = ext;
        // the grid and its bound: c1 sqrt(D) h + c2 2^20 h^2 (the header's derivation)
        const bool extent = H > 0.0 && H < inf;
        const double hs = 2.0 * (extent ? H : SD_INT_H0) / SD_INT_GRID;
        st[SD_INT] = hs;
        st[SD_INT + 1] = 1.0 / hs;
        st[SD_INT + 2] = (matern ? 0.63 : 0.61) * sqrt((double)D) * hs + (matern ? 5.0 / 6.0 : 0.5) * 2.0 * SD_INT_OFF * hs * hs;
        st[SD_INT + 3] = extent ? H : 0.0;
    }
    if ((int)threadIdx.x < D) st[SD_CTR + threadIdx.x] = sc[threadIdx.x];
}

// one workgroup per 64 rows (4 tiles of 16): thread -> (tile, lane) of every k-step
__global__ __launch_bounds__(256) void screen_dot_pack_kernel(const double* __restrict__ alpha, const double* __restrict__ Xs,
                                                              const double* __restrict__ st, double amp, int D, int ks, int n,
                                                              double* __restrict__ rows, double* __restrict__ apack) {
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63, g = l >> 4;
    const int row = tile * 16 + (l & 15);
    const bool real = row < n;
    double nb = 0.0;
    if (real)
        for (int d = 0; d < D; ++d) {
            const double b = Xs[(size_t)row * D + d] - st[SD_CTR + d];
            nb = fma(b, b, nb);
        }
    for (int kk = 0; kk < ks; ++kk) {
        const int k = 4 * kk + g;
        double v = 0.0;
        if (real && k < D) v = -2.0 * (Xs[(size_t)row * D + k] - st[SD_CTR + k]);
        rows[((size_t)tile * ks + kk) * 64 + l] = v;
    }
    // lane l < 16 holds row 16 tile + l: its norm and alpha go to slot (g, r) with l = g + 4 r
    if (l < 16) {
        const int slot = (tile >> 3) * 2 * NB + (tile & 7) * 16 + (l & 3) * 4 + (l >> 2);
        apack[slot] = real ? amp * alpha[row] : 0.0;
        apack[slot + NB] = nb;
    }
}

// The integer form's operands (header: "The integer form").  A = A0 2^16 + A1 2^8 + A2 with balanced digits in [-128, 127]:
// each digit is the sign-extended low byte of what the digits below it leave.
__device__ __forceinline__ void screen_int_digits(int A, int& d0, int& d1, int& d2) {
    d2 = (int)(signed char)A;
    A = (A - d2) >> 8;
    d1 = (int)(signed char)A;
    d0 = (A - d1) >> 8;
}
// byte d & 3 of word d >> 2: dimension d
__device__ __forceinline__ void screen_int_put(v4i& v, int d, int digit) { v[d >> 2] |= (digit & 255) << (8 * (d & 3)); }

// one workgroup per 64 rows (4 tiles of 16), as the pack above:
//     rows   [tile of 16 rows][lane l]  =  16 bytes: digit g = l >> 4 of row 16 tile + (l & 15) in dimensions 0 .. 15 (g = 3: zeros)
//     alpha  [stage of 128 rows][0][row]  =  amp alpha in natural order (the rows of lane l's D registers are 4 (l >> 4) + r)
//     norms  [stage of 128 rows][1][row]  =  |A|^2, an integer below 2^50
__global__ __launch_bounds__(256) void screen_int_pack_kernel(const double* __restrict__ alpha, const double* __restrict__ Xs,
                                                              const double* __restrict__ st, double amp, int D, int n,
                                                              v4i* __restrict__ rows, double* __restrict__ apack) {
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63, g = l >> 4;
    const int row = tile * 16 + (l & 15);
    const bool real = row < n;
    v4i v = {0, 0, 0, 0};
    double na = 0.0;
    if (real)
        for (int d = 0; d < D; ++d) {
            // (|q| <= GRID / 2 by the choice of h; the clamp keeps a fit whose rows are not finite inside the digits' range)
            const double q = fmax(fmin(rint((Xs[(size_t)row * D + d] - st[SD_CTR + d]) * st[SD_INT + 1]), SD_INT_AMAX), -SD_INT_AMAX);
            int dg[3];
            screen_int_digits((int)q, dg[0], dg[1], dg[2]);
            if (g < 3) screen_int_put(v, d, dg[g]);
            na = fma(q, q, na);
        }
    rows[(size_t)tile * 64 + l] = v;
    if (g == 0) {
        const int slot = (tile >> 3) * 2 * NB + (tile & 7) * 16 + l;
        apack[slot] = real ? amp * alpha[row] : 0.0;
        apack[slot + NB] = na;
    }
}

// sqrt(5 r2) and exp(-s) as kern_math.h's pos_sqrt / exp_nonpos, less their two selects: r2 arrives clamped at SD_R2_MIN > 0
// (rsq stays finite, s = 1e-145, k = 1 to the last bit), and 2^n underflows to 0 through v_ldexp_f64 by itself
constexpr double SD_R2_MIN = 1e-290;
template <int KIND>
__device__ __forceinline__ void screen_dot_finish(const v4d acc, double nc, const double* __restrict__ al, double (&dot)[4]) {
    double x[4], q[4];       // exp's argument (<= 0); the factor in front of it
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        // r2 = acc + |a|^2 inside the product that follows anyway (nc arrives times 5, times -1/2), the clamp behind it
        if (KIND == ROBO_KERNEL_MATERN52_ARD) {
            const double t = fmax(fma(5.0, acc[r], nc), 5.0 * SD_R2_MIN);
            double y = __builtin_amdgcn_rsq(t);
            const double e = fma(-t * y, y, 1.0);
            y = fma(y * e, fma(e, 0.375, 0.5), y);
            const double s0 = t * y;
            const double s = fma(fma(-s0, s0, t), 0.5 * y, s0);
            x[r] = -s;
            q[r] = fma(t, 1.0 / 3.0, 1.0 + s);
        } else {
            x[r] = fmin(fma(-0.5, acc[r], nc), -0.5 * SD_R2_MIN);
            q[r] = 1.0;
        }
    }
    double nn[4], rr[4], p[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        nn[r] = rint(x[r] * 1.4426950408889634074);
        rr[r] = fma(nn[r], -6.93147180369123816490e-01, x[r]);
        rr[r] = fma(nn[r], -1.90821492927058770002e-10, rr[r]);
        p[r] = 2.08767569878680989792e-09;
    }
    // Horner, one coefficient over the four rows: the constant is one scalar operand of four independent v_fma_f64
#define ROBO_SD_HORNER(C)                                     \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) p[r] = fma(p[r], rr[r], C)
    ROBO_SD_HORNER(2.50521083854417187751e-08);
    ROBO_SD_HORNER(2.75573192239858906526e-07);
    ROBO_SD_HORNER(2.75573192239858906526e-06);
    ROBO_SD_HORNER(2.48015873015873015873e-05);
    ROBO_SD_HORNER(1.98412698412698412698e-04);
    ROBO_SD_HORNER(1.38888888888888888889e-03);
    ROBO_SD_HORNER(8.33333333333333333333e-03);
    ROBO_SD_HORNER(4.16666666666666666667e-02);
    ROBO_SD_HORNER(1.66666666666666666667e-01);
    ROBO_SD_HORNER(0.5);
    ROBO_SD_HORNER(1.0);
    ROBO_SD_HORNER(1.0);
#undef ROBO_SD_HORNER
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double kv = ldexp(p[r], (int)nn[r]);
        if (KIND == ROBO_KERNEL_MATERN52_ARD) kv *= q[r];
        dot[r] = fma(kv, al[r], dot[r]);
    }
}

// The lean finish (header: "The lean finish"): the same covariance to SD_LEAN_EPS amp, not to the last bit.  One third-order
// correction of the rsq seed and no residual step, one ln 2 constant, degree 8 (tools/exp_lean_coeffs.py printed the literals).
// rint / cvt / ldexp stay: the add-and-subtract constant for n with an integer add into the exponent word for 2^n (and the
// clamp of x that form needs) was built and measured no faster (NOTES.md "The screen's lean finish and folded launches").
constexpr double SD_LEAN_EPS = 8e-13;
constexpr double SCREEN_LEAN_SAFETY = 1e4;
constexpr double SCREEN_LEAN_MAX = 1e-2;      // of the prior standard deviation: the most the lean term may add to delta
template <int KIND>
__device__ __forceinline__ void screen_dot_finish_lean(const v4d acc, double nc, const double* __restrict__ al, double (&dot)[4]) {
    double x[4], q[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (KIND == ROBO_KERNEL_MATERN52_ARD) {
            const double t = fmax(fma(5.0, acc[r], nc), 5.0 * SD_R2_MIN);
            double y = __builtin_amdgcn_rsq(t);
            const double e = fma(-t * y, y, 1.0);
            y = fma(y * e, fma(e, 0.375, 0.5), y);
            const double s = t * y;
            x[r] = -s;
            q[r] = fma(t, 1.0 / 3.0, 1.0 + s);
        } else {
            x[r] = fmin(fma(-0.5, acc[r], nc), -0.5 * SD_R2_MIN);
            q[r] = 1.0;
        }
    }
    double nn[4], rr[4], p[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        nn[r] = rint(x[r] * 1.4426950408889634074);
        rr[r] = fma(nn[r], -6.93147180559945286e-01, x[r]);
        p[r] = 2.47270673012491639e-05;
    }
#define ROBO_SD_HORNER(C)                                     \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) p[r] = fma(p[r], rr[r], C)
    ROBO_SD_HORNER(1.99155698002864343e-04);
    ROBO_SD_HORNER(1.38891798039418699e-03);
    ROBO_SD_HORNER(8.33326676781509339e-03);
    ROBO_SD_HORNER(4.16666642053601585e-02);
    ROBO_SD_HORNER(1.66666668867537560e-01);
    ROBO_SD_HORNER(5.00000000062317818e-01);
    ROBO_SD_HORNER(9.99999999980468957e-01);
    ROBO_SD_HORNER(9.99999999999759970e-01);
#undef ROBO_SD_HORNER
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double kv = ldexp(p[r], (int)nn[r]);
        if (KIND == ROBO_KERNEL_MATERN52_ARD) kv *= q[r];
        dot[r] = fma(kv, al[r], dot[r]);
    }
}

// The single-precision finish (header: "The single-precision first stage"): t (x) rounded to float behind the fp64 clamp, k~ from
// the bare hardware root and 2^x (kern_math.h hw_sqrt_f32 / hw_exp2_f32), back to double for the FMA with alpha.  Per pair: two
// fp64 instructions in front, two conversions, sqrt, add, fma, mul, exp, mul, and the fp64 FMA -- 11 against the lean
// finish's 27, no select.
constexpr double SD_SINGLE_EPS = 6.3e-7;
constexpr double SCREEN_SINGLE_SAFETY = 1.5;
constexpr double SCREEN_SINGLE_MAX = 0.5;     // of the prior standard deviation: the most the first stage's term may add to delta
// k~ / amp from t = 5 r2 (RBF: from x = -r2 / 2) as a float: the part both first-stage forms share
template <int KIND>
__device__ __forceinline__ float screen_single_cov(float tx) {
    if (KIND == ROBO_KERNEL_MATERN52_ARD) {
        const float s = hw_sqrt_f32(tx);
        const float q = fmaf(tx, 0.333333333f, 1.0f + s);
        return q * hw_exp2_f32(s * -1.44269504f);
    }
    return hw_exp2_f32(tx * 1.44269504f);
}

template <int KIND>
__device__ __forceinline__ void screen_dot_finish_single(const v4d acc, double nc, const double* __restrict__ al, double (&dot)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float tx = KIND == ROBO_KERNEL_MATERN52_ARD ? (float)fmax(fma(5.0, acc[r], nc), 5.0 * SD_R2_MIN)
                                                          : (float)fmin(fma(-0.5, acc[r], nc), -0.5 * SD_R2_MIN);
        dot[r] = fma((double)screen_single_cov<KIND>(tx), al[r], dot[r]);
    }
}

enum ScreenFinish { SD_FULL = 0, SD_LEAN = 1, SD_SINGLE = 2 };     // the template argument of screen_bounds_dot_kernel

constexpr int SD_CAND = 64;          // candidates per workgroup: one MFMA column tile of 16 per wave
constexpr int SD_STAGE = NB;         // training rows per LDS stage: 8 row tiles, swept by every wave

// Same arguments as screen_bounds_kernel, read in the dot form's layout: Xs = the packed rows, alpha = the packed amp alpha
// and norms, alpha_norm = the block [sum_j |alpha_j| sqrt(k_jj), sum_j |alpha_j|, max_j |b_j|^2, -, centre].  A wave holds its 16
// candidates' centred coordinates as the B operand for the whole sweep; a lane owns 4 training rows x 1 candidate of every
// 16 x 16 pair tile and finishes the tile while the matrix pipe forms the next one.
template <int KIND, int KS, ScreenFinish FINISH>
__global__ __launch_bounds__(256) void screen_bounds_dot_kernel(const double* __restrict__ Xcs, const double* __restrict__ Xs,
                                                                const double* __restrict__ alpha,
                                                                const double* __restrict__ alpha_norm, CovParams cp, int n,
                                                                long long m, double mean_c, double y_mean, double y_std,
                                                                int acq_kind, double par, double eta, double* __restrict__ up,
                                                                double* __restrict__ lo, unsigned long long* __restrict__ bkey) {
    __shared__ double sMx[4];
    constexpr int TILES = SD_STAGE / 16, STAGE_DOUBLES = TILES * KS * 64, PER = STAGE_DOUBLES / 256;
    __shared__ double sA[STAGE_DOUBLES];
    __shared__ __attribute__((aligned(32))) double sAN[2 * SD_STAGE];      // amp alpha | norms of the stage's rows
    const double *sAl = sAN, *sNj = sAN + SD_STAGE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, D = cp.dim;
    const long long i = (long long)blockIdx.x * SD_CAND + wave * 16 + (lane & 15);
    const bool live = i < m;
    const long long ii = live ? i : 0;
    // B fragments: the centred candidate; its norm enters in the finish
    double b[KS], nc = 0.0;
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
        const int k = 4 * kk + g;
        b[kk] = k < D ? Xcs[ii * D + k] - alpha_norm[SD_CTR + k] : 0.0;
        nc = fma(b[kk], b[kk], nc);
    }
    nc += __shfl_xor(nc, 16);
    nc += __shfl_xor(nc, 32);
    const double ncf = KIND == ROBO_KERNEL_MATERN52_ARD ? 5.0 * nc : -0.5 * nc;
    const int nst = (n + SD_STAGE - 1) / SD_STAGE;
    double pa[PER];
#pragma unroll
    for (int e = 0; e < PER; ++e) pa[e] = Xs[e * 256 + tid];
    double pan = alpha[tid];
    double dot[4] = {0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < nst; ++s) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < PER; ++e) sA[e * 256 + tid] = pa[e];
        sAN[tid] = pan;
        __syncthreads();
        if (s + 1 < nst) {
            const double* nx = Xs + (size_t)(s + 1) * STAGE_DOUBLES;
#pragma unroll
            for (int e = 0; e < PER; ++e) pa[e] = nx[e * 256 + tid];
            pan = alpha[(s + 1) * 2 * SD_STAGE + tid];
        }
        const double* nj = sNj + g * 4;
        v4d acc = v4d{nj[0], nj[1], nj[2], nj[3]};
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) acc = mfma_f64(sA[kk * 64 + lane], b[kk], acc);
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
            v4d nxt = acc;
            if (t + 1 < TILES) {
                nj += 16;
                nxt = v4d{nj[0], nj[1], nj[2], nj[3]};
#pragma unroll
                for (int kk = 0; kk < KS; ++kk) nxt = mfma_f64(sA[((t + 1) * KS + kk) * 64 + lane], b[kk], nxt);
            }
            if (FINISH == SD_SINGLE) screen_dot_finish_single<KIND>(acc, ncf, sAl + t * 16 + g * 4, dot);
            else if (FINISH == SD_LEAN) screen_dot_finish_lean<KIND>(acc, ncf, sAl + t * 16 + g * 4, dot);
            else screen_dot_finish<KIND>(acc, ncf, sAl + t * 16 + g * 4, dot);
            acc = nxt;
        }
    }
    // the candidate's four row groups in a fixed order (every lane of the four ends with the same bits)
    double mu = (dot[0] + dot[1]) + (dot[2] + dot[3]);
    mu += __shfl_xor(mu, 16);
    mu += __shfl_xor(mu, 32);
    double lmax = -__builtin_huge_val();
    if (g == 0 && live) {
        const double kself = cp.amp;
        double mt = mu + mean_c;
        mt = mt * y_std + y_mean;
        const double v_prior = kself * (y_std * y_std);
        const double ck = KIND == ROBO_KERNEL_MATERN52_ARD ? 5.0 / 6.0 : 0.5;
        const double r2_err = (double)(4 * KS + 6) * 4.44089209850062616e-16 * (nc + alpha_norm[2]);
        double delta = SCREEN_DELTA_REL * (fabs(y_mean) + fabs(y_std) * (fabs(mean_c) + sqrt(fabs(kself)) * alpha_norm[0])) +
                       SCREEN_DOT_SAFETY * fabs(y_std) * fabs(cp.amp) * ck * r2_err * alpha_norm[1];
        if (FINISH != SD_FULL) delta += SCREEN_LEAN_SAFETY * SD_LEAN_EPS * fabs(y_std) * fabs(cp.amp) * alpha_norm[1];
        if (FINISH == SD_SINGLE) delta += SCREEN_SINGLE_SAFETY * SD_SINGLE_EPS * fabs(y_std) * fabs(cp.amp) * alpha_norm[1];
        double u, l;
        screen_bounds(acq_kind, par, eta, mt, delta, v_prior, u, l);
        up[i] = u;
        lo[i] = l;
        if (!isnan(l)) lmax = l;
    }
    lmax = screen_block_max(lmax, sMx);
    if (tid == 0) atomicMax(bkey, screen_key(lmax));
}

// ---- the first stage's bounds, integer form (header: "The integer form") -------------------------------------------------------
// The same arguments, workgroup shape, stage loop and reduction as screen_bounds_dot_kernel<KIND, 4, SD_SINGLE>; Xs = the int8
// rows, alpha = the integer form's amp alpha and |A|^2.  A wave holds its 16 candidates' digits as the B operands of the four
// levels for the whole sweep; per 16 x 16 pair tile one 16-byte LDS read and four v_mfma_i32_16x16x64_i8.  Per pair, in front of
// the conversion to float: T0 = 256 S0 + S1, T1 = 256 S2 + S3 (v_lshl_add_u32), two conversions, P = 2^16 T0 + T1, |A|^2 + |B|^2,
// u = that - 512 P, t = 5 h^2 u: every value an integer below 2^53 up to the last product.
template <int KIND>
__global__ __launch_bounds__(256) void screen_bounds_dot_int_kernel(const double* __restrict__ Xcs, const v4i* __restrict__ Xs,
                                                                    const double* __restrict__ alpha,
                                                                    const double* __restrict__ alpha_norm, CovParams cp, int n,
                                                                    long long m, double mean_c, double y_mean, double y_std,
                                                                    int acq_kind, double par, double eta, double* __restrict__ up,
                                                                    double* __restrict__ lo, unsigned long long* __restrict__ bkey) {
    __shared__ double sMx[4];
    constexpr int TILES = SD_STAGE / 16, STAGE_VECS = TILES * 64, PER = STAGE_VECS / 256;
    __shared__ v4i sA[STAGE_VECS];
    __shared__ __attribute__((aligned(32))) double sAN[2 * SD_STAGE];      // amp alpha | |A|^2 of the stage's rows
    const double *sAl = sAN, *sNj = sAN + SD_STAGE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, D = cp.dim;
    const long long i = (long long)blockIdx.x * SD_CAND + wave * 16 + (lane & 15);
    const bool live = i < m;
    const long long ii = live ? i : 0;
    // the candidate's digits (every lane of a column forms all three); a coordinate beyond the digits' range is clamped and
    // marks the candidate FAR, a NaN or infinite one marks it LOST: its own term of delta below
    const double inv_h = alpha_norm[SD_INT + 1];
    v4i B0 = {0, 0, 0, 0}, B1 = {0, 0, 0, 0}, B2 = {0, 0, 0, 0};
    double nb = SD_INT_OFF;
    bool far = false, lost = false;
#pragma unroll
    for (int d = 0; d < SD_INT_MAX_D; ++d) {
        if (d < D) {
            const double q = rint((Xcs[ii * D + d] - alpha_norm[SD_CTR + d]) * inv_h);
            const bool fin = fabs(q) < __builtin_huge_val();            // false for NaN and the infinities
            const double qc = fin ? fmax(fmin(q, SD_INT_AMAX), -SD_INT_AMAX) : 0.0;
            lost = lost || !fin;
            far = far || qc != q;
            int d0, d1, d2;
            screen_int_digits((int)qc, d0, d1, d2);
            screen_int_put(B0, d, d0);
            screen_int_put(B1, d, d1);
            screen_int_put(B2, d, d2);
            nb = fma(qc, qc, nb);
        }
    }
    // the four levels' B operands: lane group g of the rows holds digit g, so level S_k pairs it with digit k - g
    const v4i zero = {0, 0, 0, 0};
    const v4i bop0 = g == 0 ? B0 : zero;
    const v4i bop1 = g == 0 ? B1 : g == 1 ? B0 : zero;
    const v4i bop2 = g == 0 ? B2 : g == 1 ? B1 : g == 2 ? B0 : zero;
    const v4i bop3 = g == 1 ? B2 : g == 2 ? B1 : zero;
    const double hs = alpha_norm[SD_INT];
    const double scale = KIND == ROBO_KERNEL_MATERN52_ARD ? 5.0 * hs * hs : -0.5 * hs * hs;
    const int nst = (n + SD_STAGE - 1) / SD_STAGE;
    v4i pa[PER];
#pragma unroll
    for (int e = 0; e < PER; ++e) pa[e] = Xs[e * 256 + tid];
    double pan = alpha[tid];
    double dot[4] = {0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < nst; ++s) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < PER; ++e) sA[e * 256 + tid] = pa[e];
        sAN[tid] = pan;
        __syncthreads();
        if (s + 1 < nst) {
            const v4i* nx = Xs + (size_t)(s + 1) * STAGE_VECS;
#pragma unroll
            for (int e = 0; e < PER; ++e) pa[e] = nx[e * 256 + tid];
            pan = alpha[(s + 1) * 2 * SD_STAGE + tid];
        }
        v4i a = sA[lane];
        v4i s0 = mfma_i8(a, bop0, zero), s1 = mfma_i8(a, bop1, zero), s2 = mfma_i8(a, bop2, zero), s3 = mfma_i8(a, bop3, zero);
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
            v4i n0 = s0, n1 = s1, n2 = s2, n3 = s3;
            if (t + 1 < TILES) {
                a = sA[(t + 1) * 64 + lane];
                n0 = mfma_i8(a, bop0, zero);
                n1 = mfma_i8(a, bop1, zero);
                n2 = mfma_i8(a, bop2, zero);
                n3 = mfma_i8(a, bop3, zero);
            }
            const double* nj = sNj + t * 16 + g * 4;
            const double* al = sAl + t * 16 + g * 4;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int t0 = s0[r] * 256 + s1[r], t1 = s2[r] * 256 + s3[r];
                const double p = fma((double)t0, 65536.0, (double)t1);
                const double u = fma(p, -512.0, nj[r] + nb);
                dot[r] = fma((double)screen_single_cov<KIND>((float)(u * scale)), al[r], dot[r]);
            }
            s0 = n0;
            s1 = n1;
            s2 = n2;
            s3 = n3;
        }
    }
    double mu = (dot[0] + dot[1]) + (dot[2] + dot[3]);
    mu += __shfl_xor(mu, 16);
    mu += __shfl_xor(mu, 32);
    double lmax = -__builtin_huge_val();
    if (g == 0 && live) {
        const double kself = cp.amp;
        double mt = mu + mean_c;
        mt = mt * y_std + y_mean;
        const double v_prior = kself * (y_std * y_std);
        // |k~ - k| / amp: the grid's bound; 1 for a clamped candidate (both lie in [0, 1]); NaN for a lost one: a survivor
        const double eps_c = lost ? __builtin_nan("") : far ? 1.0 : alpha_norm[SD_INT + 2];
        const double delta = SCREEN_DELTA_REL * (fabs(y_mean) + fabs(y_std) * (fabs(mean_c) + sqrt(fabs(kself)) * alpha_norm[0])) +
                             (SCREEN_LEAN_SAFETY * SD_LEAN_EPS + SCREEN_SINGLE_SAFETY * (SD_SINGLE_EPS + eps_c)) * fabs(y_std) *
                                 fabs(cp.amp) * alpha_norm[1];
        double u, l;
        screen_bounds(acq_kind, par, eta, mt, delta, v_prior, u, l);
        up[i] = u;
        lo[i] = l;
        if (!isnan(l)) lmax = l;
    }
    lmax = screen_block_max(lmax, sMx);
    if (tid == 0) atomicMax(bkey, screen_key(lmax));
}

// ---- survivors: count per 256 candidates, offsets, ordered gather ---------------------------------------------------------------
// candidate c is pruned only if `U_c < b` evaluates true
__device__ __forceinline__ bool screen_survives(const double* __restrict__ up, long long c, long long m, double b) {
    return c < m && !(up[c] < b);
}

// one workgroup: cnt[0 .. n_part) -> exclusive offsets, cnt[n_part] = the total; (total, b) -> pinned host memory
__device__ __forceinline__ void screen_scan(int* cnt, int n_part, double b, double* __restrict__ host) {
    __shared__ int s[256];
    __shared__ int carry;
    const int t = threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n_part; base += 256) {
        const int x = base + t < n_part ? cnt[base + t] : 0;
        s[t] = x;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int y = t >= o ? s[t - o] : 0;
            __syncthreads();
            s[t] += y;
            __syncthreads();
        }
        const int c0 = carry;
        if (base + t < n_part) cnt[base + t] = c0 + s[t] - x;
        __syncthreads();
        if (t == 255) carry = c0 + s[255];
        __syncthreads();
    }
    if (t == 0) {
        cnt[n_part] = carry;
        host[0] = (double)carry;
        host[1] = b;
    }
}

// Count and scan in one launch: every workgroup writes its count and draws a ticket (cnt[n_part + 1], zero between launches);
// the one that draws the last ticket finds every count written (fence before the ticket, fence behind it), runs the scan and
// puts the ticket back to zero.  No workgroup waits for another.
__global__ __launch_bounds__(256) void screen_count_scan_kernel(const double* __restrict__ up, long long m,
                                                                const unsigned long long* __restrict__ bkey, int* cnt,
                                                                int n_part, double* __restrict__ host) {
    __shared__ int sw[4];
    __shared__ int last;
    const double b = screen_unkey(*bkey);
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long mask = __ballot(screen_survives(up, c, m, b) ? 1 : 0);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = __builtin_popcountll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        cnt[blockIdx.x] = (sw[0] + sw[1]) + (sw[2] + sw[3]);
        __threadfence();
        last = atomicAdd(cnt + n_part + 1, 1) == n_part - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    screen_scan(cnt, n_part, b, host);
    if (threadIdx.x == 0) cnt[n_part + 1] = 0;
}

// the survivors' scaled rows in ascending original index -> sub_Xcs, their indices -> map
// The workgroup that writes row 0 also writes the pad rows rows .. cap - 1 with the same values (pad rows replicate row 0, as
// in every candidate handle; one thread doing it alone took 110 us at config 2), and the launch zeroes `clear_words` words at `clear`: the state block of the chained solve that
// follows on the stream (0: none).
__global__ __launch_bounds__(256) void screen_gather_kernel(const double* __restrict__ up, long long m,
                                                            const unsigned long long* __restrict__ bkey,
                                                            const int* __restrict__ cnt, const double* __restrict__ Xcs, int dim,
                                                            long long rows, long long cap, double* __restrict__ sub_Xcs,
                                                            long long* __restrict__ map, unsigned* __restrict__ clear,
                                                            long long clear_words) {
    __shared__ int sw[4];
    __shared__ long long first;                 // the candidate that becomes row 0, in the workgroup that holds it (-1: elsewhere)
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < clear_words; e += (long long)gridDim.x * 256) clear[e] = 0u;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool keep = screen_survives(up, c, m, screen_unkey(*bkey));
    const unsigned long long mask = __ballot(keep ? 1 : 0);
    if (lane == 0) sw[wave] = __builtin_popcountll(mask);
    if (threadIdx.x == 0) first = -1;
    __syncthreads();
    if (keep) {
        int before = __builtin_popcountll(mask & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) before += sw[w];
        const long long dst = (long long)cnt[blockIdx.x] + before;
        if (dst < cap) {
            map[dst] = c;
            for (int d = 0; d < dim; ++d) sub_Xcs[dst * dim + d] = Xcs[c * dim + d];
            if (dst == 0) first = c;
        }
    }
    __syncthreads();
    // the pad rows, by the workgroup that wrote row 0, from the same source values
    const long long c0 = first;
    if (c0 < 0) return;
    const long long total = (cap - rows) * dim;
    for (long long e = threadIdx.x; e < total; e += 256) sub_Xcs[rows * dim + e] = Xcs[c0 * dim + e % dim];
}

// the survivors' winner under its original index into the batch's own argmax slots; their flags into the batch's word.
// The gather is ascending, so the first index among equal values in the sub-batch is the first in the batch.
__global__ void screen_map_best_kernel(const double* __restrict__ sub_val, const long long* __restrict__ sub_idx,
                                       unsigned* __restrict__ sub_flags, const long long* __restrict__ map,
                                       double* __restrict__ best_val, long long* __restrict__ best_idx,
                                       unsigned* __restrict__ flags) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    *best_val = *sub_val;
    *best_idx = *sub_idx < 0 ? *sub_idx : map[*sub_idx];
    *flags |= *sub_flags;
    *sub_flags = 0u;
}

// b := max(b, best exact value of the probed candidates less rho); the probe's flags are dropped
__global__ void screen_probe_bound_kernel(const double* __restrict__ vals, const RefineSel* __restrict__ sel, int kind,
                                          unsigned long long* __restrict__ bkey, unsigned* __restrict__ probe_flags) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double best = -__builtin_huge_val();
    const int keff = (int)sel->keff;             // slots beyond the candidates with a bound hold no candidate
    for (int i = 0; i < keff; ++i)
        if (vals[i] > best) best = vals[i];
    if (kind != ROBO_ACQ_LCB) best = screen_widen(best, -1.0, kind == ROBO_ACQ_LOG_EI ? 1.0 : 0.0);
    if (best > screen_unkey(*bkey)) *bkey = screen_key(best);
    *probe_flags = 0u;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static bool screen_kind_ok(int kind, double par, double eta) {
    if (!std::isfinite(par)) return false;
    if (kind == ROBO_ACQ_LCB) return par >= 0.0;
    return (kind == ROBO_ACQ_EI || kind == ROBO_ACQ_LOG_EI || kind == ROBO_ACQ_PI) && std::isfinite(eta);
}

// alpha = L^-T z of the factor the handle holds: once per fit_gen
// the dot kernel's k-steps for this GP (0: not a kind or a D it takes); its per-fit block behind alpha's:
// [scalars and centre (SD_CTR + SCREEN_DOT_MAX_D) | packed amp alpha and norms (2 n_pad_max) | packed rows (n_pad_max x 4 KS)]
static int screen_dot_ks(const robo_gp* g) {
    if ((g->kind != ROBO_KERNEL_MATERN52_ARD && g->kind != ROBO_KERNEL_RBF_ARD) || g->dim > SCREEN_DOT_MAX_D) return 0;
    return g->dim <= 4 ? 1 : g->dim <= 8 ? 2 : g->dim <= 16 ? 4 : 8;
}

static int alpha_ensure(robo_gp* g) {
    const size_t np = (size_t)g->n_pad_max;
    const int ks = screen_dot_ks(g);
    // ... and, for D <= SD_INT_MAX_D, the integer form's [amp alpha and |A|^2 (2 n_pad_max) | int8 rows (n_pad_max x 64 bytes)]
    const bool ints = ks && g->dim <= SD_INT_MAX_D;
    const size_t dot_doubles = ks ? SD_STATS + 2 * np + np * 4 * (size_t)ks + (ints ? 2 * np + 8 * np : 0) : 0;
    if (!g->d_alpha) ROBO_TRY(dev_alloc(&g->d_alpha, 2 * np + 8 + dot_doubles));
    if (g->alpha_gen == g->fit_gen) return ROBO_OK;
    robo_ctx* c = g->ctx;
    hipStream_t st = c->stream;
    double* v = g->d_alpha;
    double* a = g->d_alpha + np;
    ROBO_HIP_CHECK(hipMemcpyAsync(v, g->d_K + (size_t)g->n * g->n_pad, (size_t)g->n * sizeof(double), hipMemcpyDeviceToDevice, st));
    ROBO_TRY(launch_bwd_rows(g, v, a));
    double* stats = g->d_alpha + 2 * np;
    hipLaunchKernelGGL(screen_alpha_norm_kernel, dim3(1), dim3(256), 0, st, (const double*)a, (const double*)g->d_Xs, g->cov,
                       g->n, stats);
    g->dot_extent = g->dot_alpha_sum = g->int_step = g->int_eps = 0.0;
    if (ks) {
        double* apack = stats + SD_STATS;
        const int nst = (g->n + SD_STAGE - 1) / SD_STAGE;
        hipLaunchKernelGGL(screen_dot_prep_kernel, dim3(1), dim3(256), 0, st, (const double*)a, (const double*)g->d_Xs, g->dim,
                           g->n, g->kind == ROBO_KERNEL_MATERN52_ARD ? 1 : 0, stats);
        hipLaunchKernelGGL(screen_dot_pack_kernel, dim3((unsigned)(nst * SD_STAGE / 64)), dim3(256), 0, st, (const double*)a,
                           (const double*)g->d_Xs, (const double*)stats, g->cov.amp, g->dim, ks, g->n, apack + 2 * np, apack);
        if (ints) {
            double* ipack = apack + 2 * np + np * 4 * (size_t)ks;
            hipLaunchKernelGGL(screen_int_pack_kernel, dim3((unsigned)(nst * SD_STAGE / 64)), dim3(256), 0, st, (const double*)a,
                               (const double*)g->d_Xs, (const double*)stats, g->cov.amp, g->dim, g->n,
                               reinterpret_cast<v4i*>(ipack + 2 * np), ipack);
        }
        ROBO_LAUNCH_CHECK();
        // the centred extent decides between the two kernels on the host, sum_j |alpha_j| between the finishes, the grid's
        // bound between the first stage's two forms: one small copy per fit_gen
        static_assert(SD_STATS - 1 <= 48, "the pinned block's tail");
        double* hp = c->h_pinned + MAX_DIM + 16;
        ROBO_HIP_CHECK(hipMemcpyAsync(hp, stats + 1, (SD_STATS - 1) * sizeof(double), hipMemcpyDeviceToHost, st));
        ROBO_HIP_CHECK(hipStreamSynchronize(st));
        g->dot_alpha_sum = hp[0];
        g->dot_extent = hp[2];
        if (ints) {
            g->int_step = hp[SD_INT - 1];
            g->int_eps = hp[SD_INT + 3 - 1] > 0.0 ? hp[SD_INT + 2 - 1] : 0.0;      // no extent: no rule-admitted grid
        }
    }
    ROBO_LAUNCH_CHECK();
    g->alpha_gen = g->fit_gen;
    return ROBO_OK;
}

// whether the bounds of this factor come from the dot kernel (header: "Selection"); alpha_ensure has run
static bool screen_dot_wanted(const robo_gp* g) {
    const int t = g->ctx->tune.acq_screen_dot;
    if (t == 0 || !screen_dot_ks(g)) return false;
    if (t > 0) return true;
    const double worst = (double)(g->dim + 3) * 4.44089209850062616e-16 * g->dot_extent;
    return worst <= SCREEN_DOT_BOUND;            // (a NaN extent takes the direct kernel)
}

// whether the dot kernel finishes its pairs with the lean finish (header: "The lean finish"); alpha_ensure has run
static bool screen_lean_wanted(const robo_gp* g) {
    const int t = g->ctx->tune.acq_screen_lean;
    if (t == 0) return false;
    if (t > 0) return true;
    // the term the finish adds to delta, in units of the prior standard deviation |y_std| sqrt(amp)
    const double term = SCREEN_LEAN_SAFETY * SD_LEAN_EPS * std::sqrt(std::fabs(g->cov.amp)) * g->dot_alpha_sum;
    return term <= SCREEN_LEAN_MAX;              // (a NaN sum takes the full finish)
}

// whether this factor's argmax-only calls may form their bounds with the single-precision finish first (header: "The
// single-precision first stage"; the pause is acq_sweep_best's); alpha_ensure has run
static bool screen_single_wanted(const robo_gp* g) {
    const int t = g->ctx->tune.acq_screen_single;
    if (t == 0 || !screen_dot_wanted(g) || !screen_lean_wanted(g)) return false;
    if (t > 0) return true;
    const double term = SCREEN_SINGLE_SAFETY * SD_SINGLE_EPS * std::sqrt(std::fabs(g->cov.amp)) * g->dot_alpha_sum;
    return term <= SCREEN_SINGLE_MAX;            // (a NaN sum: no first stage)
}

// whether that first stage takes its squared distances from the int8 products (header: "The integer form"); the caller has
// asked screen_single_wanted
static bool screen_int_wanted(const robo_gp* g) {
    const int t = g->ctx->tune.acq_screen_int;
    if (t == 0 || g->dim > SD_INT_MAX_D || !(g->int_step > 0.0)) return false;
    if (t > 0) return true;
    // measured: at D <= 8 the fp64 form needs one or two k-steps per pair tile and the integer form's four products and six
    // more instructions per pair do not clear the rule (config 2: 53.1 against 54.1 us); it pays from four k-steps on
    if (screen_dot_ks(g) != 4) return false;
    if (!(g->int_eps > 0.0)) return false;       // rows without an extent: no grid of their own
    const double term = SCREEN_SINGLE_SAFETY * (SD_SINGLE_EPS + g->int_eps) * std::sqrt(std::fabs(g->cov.amp)) * g->dot_alpha_sum;
    return term <= SCREEN_SINGLE_MAX;            // (a NaN sum: the fp64-MFMA form, under its own rule)
}

static int screen_buffers(robo_cand* k) {
    const size_t mp = (size_t)k->m_pad;
    if (!k->d_scr_up) ROBO_TRY(dev_alloc(&k->d_scr_up, mp));
    if (!k->d_scr_lo) ROBO_TRY(dev_alloc(&k->d_scr_lo, mp + 2));    // bounds | b (as its order-preserving key)
    if (!k->d_scr_cnt) {
        // counts -> offsets | total | the ticket of screen_count_scan_kernel, zero between launches
        ROBO_TRY(dev_alloc(&k->d_scr_cnt, (size_t)k->n_part + 2));
        ROBO_HIP_CHECK(hipMemsetAsync(k->d_scr_cnt, 0, ((size_t)k->n_part + 2) * sizeof(int), k->ctx->stream));
    }
    return ROBO_OK;
}

// scaled rows of k and the bounds of every candidate into k->d_scr_up / d_scr_lo (asynchronous); `single`: with the
// single-precision finish (the caller has asked screen_single_wanted).  scr_finish reports the fp64 finish selected for the
// factor either way
static int launch_screen_bounds(robo_gp* g, robo_cand* k, int kind, double par, double eta, bool single = false) {
    robo_ctx* c = g->ctx;
    ROBO_TRY(alpha_ensure(g));
    ROBO_TRY(screen_buffers(k));
    unsigned long long* bkey = reinterpret_cast<unsigned long long*>(k->d_scr_lo + k->m_pad);
    ROBO_TRY(launch_scale_inputs(c, k->d_Xc, k->d_Xcs, g->d_theta, k->m, k->m_pad, g->dim, 1, 0, 0, bkey, SCREEN_KEY_NONE));
    const dim3 grid((unsigned)((k->m + SC_CAND - 1) / SC_CAND));
    const double* alpha = g->d_alpha + (size_t)g->n_pad_max;
    const double* anorm = g->d_alpha + 2 * (size_t)g->n_pad_max;
    k->scr_int = 0;
    k->scr_int_step = 0.0;
    if (screen_dot_wanted(g)) {
        const double* apack = anorm + SD_STATS;
        const double* rows = apack + 2 * (size_t)g->n_pad_max;
        const dim3 dgrid((unsigned)((k->m + SD_CAND - 1) / SD_CAND));
        if (single && screen_int_wanted(g)) {
            // the first stage's integer form; reported as the dot kernel's family (robo_cand_last_screen_form tells the form)
            const double* ipack = rows + (size_t)g->n_pad_max * 4 * screen_dot_ks(g);
            const v4i* irows = reinterpret_cast<const v4i*>(ipack + 2 * (size_t)g->n_pad_max);
#define ROBO_SCREEN_INT_CALL(KIND)                                                                                              \
    hipLaunchKernelGGL((screen_bounds_dot_int_kernel<KIND>), dgrid, dim3(256), 0, c->stream, (const double*)k->d_Xcs, irows, ipack, \
                       anorm, g->cov, g->n, (long long)k->m, g->mean_c, g->y_mean, g->y_std, kind, par, eta, k->d_scr_up,      \
                       k->d_scr_lo, bkey)
            if (g->kind == ROBO_KERNEL_MATERN52_ARD) ROBO_SCREEN_INT_CALL(ROBO_KERNEL_MATERN52_ARD);
            else ROBO_SCREEN_INT_CALL(ROBO_KERNEL_RBF_ARD);
#undef ROBO_SCREEN_INT_CALL
            ROBO_LAUNCH_CHECK();
            k->scr_bounds_kernel = "screen_bounds_dot_kernel";
            k->scr_finish = screen_lean_wanted(g) ? ROBO_SCREEN_FINISH_LEAN : ROBO_SCREEN_FINISH_FULL;
            k->scr_int = 1;
            k->scr_int_step = g->int_step;
            return ROBO_OK;
        }
#define ROBO_SCREEN_DOT_CALL(KIND, KS, LEAN)                                                                                  \
    hipLaunchKernelGGL((screen_bounds_dot_kernel<KIND, KS, LEAN>), dgrid, dim3(256), 0, c->stream, (const double*)k->d_Xcs, rows,  \
                       apack, anorm, g->cov, g->n, (long long)k->m, g->mean_c, g->y_mean, g->y_std, kind, par, eta,          \
                       k->d_scr_up, k->d_scr_lo, bkey)
#define ROBO_SCREEN_DOT_KS(KIND, LEAN)                            \
    switch (screen_dot_ks(g)) {                                   \
        case 1: ROBO_SCREEN_DOT_CALL(KIND, 1, LEAN); break;       \
        case 2: ROBO_SCREEN_DOT_CALL(KIND, 2, LEAN); break;       \
        case 4: ROBO_SCREEN_DOT_CALL(KIND, 4, LEAN); break;       \
        default: ROBO_SCREEN_DOT_CALL(KIND, 8, LEAN); break;      \
    }
        const bool lean = screen_lean_wanted(g);
        if (g->kind == ROBO_KERNEL_MATERN52_ARD) {
            if (single) ROBO_SCREEN_DOT_KS(ROBO_KERNEL_MATERN52_ARD, SD_SINGLE)
            else if (lean) ROBO_SCREEN_DOT_KS(ROBO_KERNEL_MATERN52_ARD, SD_LEAN)
            else ROBO_SCREEN_DOT_KS(ROBO_KERNEL_MATERN52_ARD, SD_FULL)
        } else {
            if (single) ROBO_SCREEN_DOT_KS(ROBO_KERNEL_RBF_ARD, SD_SINGLE)
            else if (lean) ROBO_SCREEN_DOT_KS(ROBO_KERNEL_RBF_ARD, SD_LEAN)
            else ROBO_SCREEN_DOT_KS(ROBO_KERNEL_RBF_ARD, SD_FULL)
        }
#undef ROBO_SCREEN_DOT_KS
#undef ROBO_SCREEN_DOT_CALL
        ROBO_LAUNCH_CHECK();
        k->scr_bounds_kernel = "screen_bounds_dot_kernel";
        k->scr_finish = lean ? ROBO_SCREEN_FINISH_LEAN : ROBO_SCREEN_FINISH_FULL;
        return ROBO_OK;
    }
    k->scr_bounds_kernel = "screen_bounds_kernel";
    k->scr_finish = ROBO_SCREEN_FINISH_NONE;
#define ROBO_SCREEN_CALL(KIND)                                                                                           \
    do {                                                                                                                  \
        if (g->dim <= 16)                                                                                                 \
            hipLaunchKernelGGL((screen_bounds_kernel<KIND, true>), grid, dim3(256), 0, c->stream, (const double*)k->d_Xcs, \
                               (const double*)g->d_Xs, alpha, anorm, g->cov, g->n, (long long)k->m, g->mean_c, g->y_mean, \
                               g->y_std, kind, par, eta, k->d_scr_up, k->d_scr_lo, bkey);                                     \
        else                                                                                                              \
            hipLaunchKernelGGL((screen_bounds_kernel<KIND, false>), grid, dim3(256), 0, c->stream, (const double*)k->d_Xcs, \
                               (const double*)g->d_Xs, alpha, anorm, g->cov, g->n, (long long)k->m, g->mean_c, g->y_mean, \
                               g->y_std, kind, par, eta, k->d_scr_up, k->d_scr_lo, bkey);                                     \
    } while (0)
    if (g->kind == ROBO_KERNEL_MATERN52_ARD) ROBO_SCREEN_CALL(ROBO_KERNEL_MATERN52_ARD);
    else if (g->kind == ROBO_KERNEL_RBF_ARD) ROBO_SCREEN_CALL(ROBO_KERNEL_RBF_ARD);
    else ROBO_SCREEN_CALL(ROBO_KERNEL_FABOLAS);
#undef ROBO_SCREEN_CALL
    ROBO_LAUNCH_CHECK();
    return ROBO_OK;
}

// everything acq_sweep would check is in order, and the call is one the screen handles
static bool screen_eligible(const robo_gp* g, const robo_cand* k, int kind, double par, double eta) {
    if (!g || !k || !g->fitted || k->dim != g->dim || k->ctx != g->ctx) return false;
    const Tuning& t = g->ctx->tune;
    if (t.acq_screen == 0 || !screen_kind_ok(kind, par, eta)) return false;
    if (k->m <= (t.acq_screen_min >= 0 ? t.acq_screen_min : t.winv_max)) return false;
    // the unscreened call must be the fused block-row substitution: its results do not depend on the tile a candidate is in
    if (g->fp32_gram || t.predict_stepwise || winv_candidate(g, k)) return false;
    return g->diag_min > 0.0 && g->diag_max <= SCREEN_DIAG_RATIO_MAX * g->diag_min;
}

// the sub-handle of the survivors, sized once for the most the cap lets through
static int screen_sub(robo_cand* k, int64_t cap) {
    if (cap < SCREEN_PROBE) cap = SCREEN_PROBE;       // the probe's tile goes through the same sub-handle
    if (k->scr_sub && k->scr_cap >= cap) return ROBO_OK;
    robo_cand_destroy(k->scr_sub);
    hipFree(k->d_scr_map);
    k->scr_sub = nullptr;
    k->d_scr_map = nullptr;
    k->scr_cap = 0;
    ROBO_TRY(cand_alloc(k->ctx, cap, k->dim, &k->scr_sub));
    ROBO_TRY(dev_alloc(&k->d_scr_map, (size_t)k->scr_sub->m_pad));
    k->scr_cap = cap;
    return ROBO_OK;
}

int acq_sweep_best(robo_gp* g, int32_t kind, double par, double eta, robo_cand* k, bool want_values, bool allow_chain,
                   double* h_report) {
    if (k) {
        k->best_reported = false;
        k->scr_outcome = ROBO_SCREEN_NOT_ELIGIBLE;
        k->scr_n = k->scr_kept = 0;
        k->scr_tail_fused = false;
        k->scr_first_stage = 0;
        k->scr_first_kept = 0;
        k->scr_int = 0;
        k->scr_int_step = 0.0;
    }
    if (want_values || !screen_eligible(g, k, kind, par, eta)) return acq_sweep(&g, 1, false, kind, par, &eta, k, allow_chain);
    if (g->screen_gen != g->fit_gen) {
        g->screen_gen = g->fit_gen;
        g->screen_skip = 0;
        g->screen_backoff = 1;
        g->single_skip = 0;
        g->single_backoff = 1;
    }
    if (g->screen_skip > 0) {
        --g->screen_skip;
        return acq_sweep(&g, 1, false, kind, par, &eta, k, allow_chain);
    }
    robo_ctx* c = g->ctx;
    hipStream_t st = c->stream;
    ROBO_HIP_CHECK(hipSetDevice(c->device));
    k->solved_gen = 0;
    // the first stage (header: "The cascade"): the same launches with the single-precision finish, unless the factor's rule or
    // its pause says no
    ROBO_TRY(alpha_ensure(g));
    bool first = screen_single_wanted(g);
    if (first && g->single_skip > 0) {
        --g->single_skip;
        first = false;
    }
    ROBO_TRY(launch_screen_bounds(g, k, kind, par, eta, first));
    unsigned long long* b = reinterpret_cast<unsigned long long*>(k->d_scr_lo + k->m_pad);     // max_c L_c: the bounds kernel's
    double* hp = c->h_pinned + 8;
    const dim3 blocks((unsigned)k->n_part);
    // survivors of the current b: counts, offsets, the total into pinned memory (one synchronisation)
    int64_t kept = 0;
    auto count_survivors = [&]() -> int {
        hipLaunchKernelGGL(screen_count_scan_kernel, blocks, dim3(256), 0, st, (const double*)k->d_scr_up, (long long)k->m,
                           (const unsigned long long*)b, k->d_scr_cnt, k->n_part, hp);
        ROBO_LAUNCH_CHECK();
        ROBO_HIP_CHECK(hipStreamSynchronize(st));
        kept = (int64_t)hp[0];
        return ROBO_OK;
    };
    ROBO_TRY(count_survivors());
    int64_t cap = k->m / 100 * c->tune.acq_screen_keep_max + k->m % 100 * c->tune.acq_screen_keep_max / 100;
    if (cap > k->m) cap = k->m;
    if (cap < 1) cap = 1;
    if (first) {
        k->scr_first_kept = kept;
        if (kept >= 1 && kept <= (cap < NB ? cap : (int64_t)NB)) {
            // decided: on from the gather with these survivors (a superset of the fp64 pass's)
            k->scr_first_stage = 1;
            g->single_backoff = 1;
        } else {
            // the fp64 path on the whole batch, as without a first stage; the first stage pauses
            k->scr_first_stage = 2;
            g->single_skip = g->single_backoff;
            if (g->single_backoff < (1 << 20)) g->single_backoff *= 2;
            const int first_int = k->scr_int;
            const double first_step = k->scr_int_step;
            ROBO_TRY(launch_screen_bounds(g, k, kind, par, eta));
            ROBO_TRY(count_survivors());
            k->scr_int = first_int;                // the form reported is the first stage's
            k->scr_int_step = first_step;
        }
    }
    k->scr_n = k->m;
    k->scr_kept = kept;
    bool probed = false;
    if (kept > cap) {
        // the incumbent from the exact values of the candidates with the largest upper bounds
        ROBO_TRY(screen_sub(k, cap));
        if (!k->scr_probe) ROBO_TRY(refine_alloc(c, SCREEN_PROBE, k->dim, &k->scr_probe));
        const RefineState& ps = k->scr_probe->st;
        robo_cand* s = k->scr_sub;
        ROBO_TRY(launch_refine_select(c, ps, k->d_scr_up, k->m, k->d_Xcs, 0.0));
        s->m = s->m_pad = SCREEN_PROBE;
        s->n_part = 1;
        s->solved_gen = 0;
        ROBO_HIP_CHECK(hipMemcpyAsync(s->d_Xcs, ps.x, (size_t)SCREEN_PROBE * k->dim * sizeof(double), hipMemcpyDeviceToDevice, st));
        ROBO_TRY(cand_ensure_workspace(s, g->n_pad, false));
        ROBO_TRY(predict_scaled(g, s, false, nullptr, false, false, allow_chain));
        ROBO_TRY(clear_flags_on_error(s, launch_acq(c, s, kind, par, eta, false, false)));
        hipLaunchKernelGGL(screen_probe_bound_kernel, dim3(1), dim3(64), 0, st, (const double*)s->d_acq,
                           (const RefineSel*)ps.sel, kind, b, s->d_flags);
        ROBO_LAUNCH_CHECK();
        ROBO_TRY(count_survivors());
        // (a probe whose chained solve gave up has produced no incumbent: the caller starts over, on launches)
        if (allow_chain && chain_timed_out(c)) return clear_flags_on_error(s, ROBO_CHAIN_RETRY);
        k->scr_kept = kept;
        probed = true;
    }
    if (kept < 1 || kept > cap) {
        // nothing to gain on this factor for now: the plain sweep, and a pause that doubles with every failed screen
        k->scr_outcome = ROBO_SCREEN_FELL_BACK;
        g->screen_skip = g->screen_backoff;
        if (g->screen_backoff < (1 << 20)) g->screen_backoff *= 2;
        return acq_sweep(&g, 1, false, kind, par, &eta, k, allow_chain);
    }
    g->screen_backoff = 1;
    k->scr_outcome = probed ? ROBO_SCREEN_PROBE_USED : ROBO_SCREEN_SCREENED;
    ROBO_TRY(screen_sub(k, cap));
    robo_cand* s = k->scr_sub;
    s->m = kept;
    s->m_pad = round_up64(kept, NB);
    s->n_part = (int)((kept + 255) / 256);
    s->solved_gen = 0;
    // where the survivors' solve will be ONE chained launch, the gather zeroes its state block too (launch_predict_chain
    // then skips its memset; any other outcome keeps it)
    ROBO_TRY(cand_ensure_workspace(s, g->n_pad, false));
    unsigned* clear = nullptr;
    size_t clear_bytes = 0;
    s->chain_cleared = 0;
    if (allow_chain && s->chunk >= s->m_pad && !g->fp32_gram && !c->tune.predict_stepwise && chain_wanted(g, s->m_pad)) {
        ROBO_TRY(chain_state_ensure(g, s, s->m_pad, &clear_bytes));
        clear = reinterpret_cast<unsigned*>(s->d_chain);
    }
    hipLaunchKernelGGL(screen_gather_kernel, blocks, dim3(256), 0, st, (const double*)k->d_scr_up, (long long)k->m,
                       (const unsigned long long*)b, (const int*)k->d_scr_cnt, (const double*)k->d_Xcs, k->dim, (long long)kept,
                       (long long)s->m_pad, s->d_Xcs, k->d_scr_map, clear, (long long)(clear_bytes / sizeof(unsigned)));
    ROBO_LAUNCH_CHECK();
    s->chain_cleared = clear_bytes;
    // the path the unscreened call runs for the whole batch; its event pair 25 -> 26 is the batch's (bench.py reads it)
    // survivors within one partial block: the tail is one single-workgroup launch (acq.hip acq_tail_kernel)
    const bool fused = c->tune.acq_screen_fused_tail != 0 && s->n_part == 1 && s->m_pad <= 256;
    s->defer_post = fused;
    const int solved = predict_scaled(g, s, false, nullptr, false, phase_events_on(g->ctx, k), allow_chain);
    s->chain_cleared = 0;
    s->defer_post = false;
    ROBO_TRY(solved);
    int status = fused ? launch_acq_tail(g, s, kind, par, eta, k->d_scr_map, k, h_report) : launch_acq(c, s, kind, par, eta, false, false);
    if (fused) {
        k->scr_tail_fused = true;
        if (status == ROBO_OK) k->best_reported = h_report != nullptr;
    } else if (status == ROBO_OK) {
        hipLaunchKernelGGL(screen_map_best_kernel, dim3(1), dim3(64), 0, st, (const double*)(s->d_part_val + s->n_part),
                           (const long long*)(s->d_part_idx + s->n_part), s->d_flags, (const long long*)k->d_scr_map,
                           k->d_part_val + k->n_part, k->d_part_idx + k->n_part, k->d_flags);
        if (hipGetLastError() != hipSuccess) status = ROBO_RUNTIME_ERROR;
    }
    if (status != ROBO_OK) clear_flags_on_error(s, status);
    k->solve_kernel = s->solve_kernel;
    return clear_flags_on_error(k, status);
}

}  // namespace robo

using namespace robo;

extern "C" {

int32_t robo_cand_last_screen(robo_cand* k, int64_t* out_n_screened, int64_t* out_n_survivors, int32_t* out_outcome) {
    if (!k) return ROBO_BAD_ARGUMENT;
    if (out_n_screened) *out_n_screened = k->scr_n;
    if (out_n_survivors) *out_n_survivors = k->scr_kept;
    if (out_outcome) *out_outcome = k->scr_outcome;
    return ROBO_OK;
}

int32_t robo_cand_last_screen_finish(robo_cand* k, int32_t* out_finish, int32_t* out_fused_tail) {
    if (!k || !out_finish) return ROBO_BAD_ARGUMENT;
    *out_finish = k->scr_finish;
    if (out_fused_tail) *out_fused_tail = k->scr_tail_fused ? 1 : 0;
    return ROBO_OK;
}

int32_t robo_cand_last_screen_first(robo_cand* k, int32_t* out_stage, int64_t* out_kept) {
    if (!k) return ROBO_BAD_ARGUMENT;
    if (out_stage) *out_stage = k->scr_first_stage;
    if (out_kept) *out_kept = k->scr_first_kept;
    return ROBO_OK;
}

int32_t robo_cand_last_screen_form(robo_cand* k, int32_t* out_form, double* out_step) {
    if (!k) return ROBO_BAD_ARGUMENT;
    if (out_form) *out_form = k->scr_int ? ROBO_SCREEN_FORM_INT8 : ROBO_SCREEN_FORM_FP64;
    if (out_step) *out_step = k->scr_int_step;
    return ROBO_OK;
}

int32_t robo_acq_screen_bounds(robo_gp* g, int32_t acq_kind, double par, double eta, robo_cand* k, double* out_upper,
                               double* out_lower) {
    if (!g || !k) return ROBO_BAD_ARGUMENT;
    ROBO_TRY(check_acq_kind(acq_kind));
    if (!g->fitted) {
        set_error("Model has to be trained first!");
        return ROBO_NOT_FITTED;
    }
    if (k->dim != g->dim || k->ctx != g->ctx) {
        set_error("candidate batch (dim %d) does not match the GP (dim %d) or lives on another context", k->dim, g->dim);
        return ROBO_BAD_SHAPE;
    }
    if (g->fp32_gram || !screen_kind_ok(acq_kind, par, eta)) {
        set_error("robo_acq_screen_bounds: no bound for this call (LCB needs kappa >= 0; finite eta / par; fp64 covariance "
                  "entries)");
        return ROBO_BAD_ARGUMENT;
    }
    hipStream_t st = g->ctx->stream;
    ROBO_HIP_CHECK(hipSetDevice(g->ctx->device));
    k->solved_gen = 0;
    // acq_screen_single = 2 (tests): the first stage's bounds where it would run, its pause aside
    ROBO_TRY(alpha_ensure(g));
    ROBO_TRY(launch_screen_bounds(g, k, acq_kind, par, eta, g->ctx->tune.acq_screen_single == 2 && screen_single_wanted(g)));
    if (out_upper)
        ROBO_HIP_CHECK(hipMemcpyAsync(out_upper, k->d_scr_up, (size_t)k->m * sizeof(double), hipMemcpyDeviceToHost, st));
    if (out_lower)
        ROBO_HIP_CHECK(hipMemcpyAsync(out_lower, k->d_scr_lo, (size_t)k->m * sizeof(double), hipMemcpyDeviceToHost, st));
    ROBO_HIP_CHECK(hipStreamSynchronize(st));
    return ROBO_OK;
}

}  // extern "C"
