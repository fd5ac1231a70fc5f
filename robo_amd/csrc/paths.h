// Pathwise posterior samples (paths.hip, api_paths.hip): the handle and what the host passes to the kernels.  The rule is
// stated in include/robo_hip.h.
#pragma once
#include "common.h"

namespace robo {

constexpr int PT = 64;           // tile edge: candidates per workgroup, operand rows (training points / features) per step
constexpr int PD = 16;           // dimensions per LDS pass of stage 1
constexpr int PLD = PT + 2;      // LDS leading dimension: fragment reads of stage 2 touch 32 distinct banks per half wave
constexpr int PATHS_SW = 16;     // paths per MFMA column tile

// one launch of the path kernel over rows [c0, c0 + 64 gridDim.x) of X
struct PathsArgs {
    const double* X;             // scaled rows (pad rows present), dim doubles each
    long long c0, m;             // first row of the launch; rows >= m are pads: not stored, not reduced
    const double* Xs;            // data pass: n_tiles x 64 scaled training rows, weights alpha (S_pad x ld_alpha)
    const double* alpha;
    int n_tiles, ld_alpha;
    const double* omega;         // feature pass: f_tiles x 64 frequencies (pad rows zero), phases, weights w (S_pad x ld_w)
    const double* phase;
    const double* w;
    int f_tiles, ld_w;
    int S, ns;                   // paths; column tiles of 16 paths (pad paths carry zero weights)
    CovParams cp;
    double fscale;               // sqrt(2 amp / F)
    double mean_c, y_mean, y_std;
    int raw;                     // 1: the two sums alone (no mean, no transform, no reduction): Phi_X w at the training rows
    int self;                    // 1: X is Xs itself (K alpha at the training rows): the diagonal entries are exact
    double* out;                 // S x ld_out values, column = row of X - c0; nullptr: not stored
    long long ld_out;
    double* part_val;            // S x n_part per-tile best (value, row) of every path; row -1: the tile has no live row
    long long* part_idx;
    long long n_part;
    unsigned* flags;
};

int launch_paths(robo_ctx* ctx, const PathsArgs& a, long long rows);
int launch_paths_rhs(robo_ctx* ctx, double* d_r, const double* d_y, const double* d_eps, int S, int n, int n_pad, double mean_c,
                     double sd);
// rho = r - (K alpha + noise alpha) over the training rows in place of K alpha (d_ka), 0 in the pad rows; alpha += delta
int launch_paths_residual(robo_ctx* ctx, double* d_ka, const double* d_r, const double* d_alpha, int S, int n, int n_pad,
                          double noise);
int launch_paths_add(robo_ctx* ctx, double* d_alpha, const double* d_delta, int S, int n_pad);
// alpha = L^-T L^-1 r for S right-hand sides (rows of d_r, n_pad doubles each; consumed), d_tmp of the same size
int launch_paths_solve(robo_ctx* ctx, const double* d_L, int n_pad, const double* d_Linv, int n, int S, double* d_r,
                       double* d_tmp);
int launch_paths_best(robo_ctx* ctx, const double* part_val, const long long* part_idx, long long n_part, int S, double* best_val,
                      long long* best_idx);

// ---- refinement of a path's minimiser (paths_refine.hip; the rule is stated in include/robo_hip.h) ---------------------------------
constexpr int PDG = 4;                       // descents per workgroup, one wave each (measured against 1: NOTES.md)
constexpr int PATHS_REFINE_MAX_DIM = 64;     // a descent keeps coordinate d in lane d of its wave

// one launch of the descent kernel: P descents from their starts to the last iteration
struct PathsDescentArgs {
    const double* Xs;            // data pass: scaled training rows, weights alpha (row path_of[i], ld_alpha doubles)
    const double* alpha;
    int n, ld_alpha;
    const double* omega;         // feature pass: frequencies, phases, weights w (row path_of[i], ld_w doubles)
    const double* phase;
    const double* w;
    int F, ld_w;
    const double* ism;           // the snapshot's metric: x~ = x (.) ism
    CovParams cp;
    double fscale, mean_c, y_mean, y_std;
    int P, T;
    double step0;
    const int* path_of;          // P
    const long long* start;      // P rows the starts came from (-1: the slot is unused), or nullptr: every slot is used
    const double* x0;            // P x dim starts
    double *x, *f, *g;           // P x dim, P, P x dim: the last accepted point, its value and gradient
    int* code;                   // P: the code of the last iteration
    double* trace;               // (T + 1) x P x (2 dim + 3), or nullptr
    unsigned* flags;
};

// the device state of robo_paths_descend / robo_paths_refine_cand: one block, laid out by paths_refine_ensure
struct PathsRefineState {
    double *x0, *x, *f, *g;      // PathsDescentArgs' arrays
    double* sval;                // P: the sweep's value of every start (NaN: the slot is unused)
    double* res;                 // S x (dim + 2): per path the winner's point, its value, the row its start came from
    long long* start;
    int *path_of, *code;
};

int launch_paths_descent(robo_ctx* ctx, const PathsDescentArgs& a);
// per path the n_starts smallest group bests of the sweep -> start / sval / path_of / x0 of its n_starts slots
int launch_paths_starts(robo_ctx* ctx, const double* part_val, const long long* part_idx, long long n_part, int S, int n_starts,
                        const double* Xc, int dim, const PathsRefineState& st);
// per path the descent with the smallest final value (sweep_only: the first start and the sweep's value of it) -> st.res
int launch_paths_winners(robo_ctx* ctx, int S, int n_starts, int dim, const PathsRefineState& st, bool sweep_only,
                         unsigned* flags);

}  // namespace robo

// a snapshot: nothing here points into the GP it was drawn from
struct robo_paths {
    robo_ctx* ctx;
    int kind, dim, n, n_pad, F, F_pad, S, S_pad;
    robo::CovParams cov;
    double mean_c, y_mean, y_std, fscale;
    double *d_Xs, *d_ism, *d_alpha, *d_omega, *d_phase, *d_w;
    double* d_part_val;          // S x part_cap per-tile bests, then the S winners
    long long* d_part_idx;
    size_t part_cap;
    double* d_best_val;
    long long* d_best_idx;
    unsigned* d_flags;
    char* d_refine;              // the refinement's state block (grows), laid out behind `rs`; its diagnostics trace
    size_t refine_cap;
    double* d_trace;
    size_t trace_cap;
    robo::PathsRefineState rs;
};
