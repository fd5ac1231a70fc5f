// The regression forest (forest.hip, api_forest.hip): the handle, what the host passes to the kernels and the scratch a tree
// keeps per node while it grows.  The rule is stated in include/robo_hip.h.
#pragma once
#include "blr_dev.h"

namespace robo {

constexpr int RF_MAX_N = ROBO_RF_MAX_N;
constexpr int RF_NODE_BITS = 0x1FFF;           // a row's node id in s_nid (node ids stay below 2 RF_MAX_N - 1 = 8191)
constexpr int RF_SPLIT_BIT = 0x8000;           // ... the row's node splits at this level
constexpr int RF_RIGHT_BIT = 0x4000;           // ... and the row goes right
constexpr int RF_STAGE_NODES = 768;            // sweep: a tree of at most this many nodes is walked in LDS
constexpr int RF_STAGE_COORDS = 5120;          // sweep: doubles of staged candidate coordinates per workgroup

struct RfScratch {                // per node of a growing tree; device memory, private to the tree's workgroup
    double S, best;               // sum of w y_c over the node's rows; the best score so far (< 0: none)
    int start, cnt;               // the node's segment of every feature list: [start, start + cnt)
    int bfeat, bpos;              // the best split's feature and its position inside the segment
};

struct RfGrow {                   // what the grow kernel is passed; every pointer device memory
    int n, D, T, stride, n_points, bootstrap, max_features, min_split, min_leaf, max_depth;
    double eps_purity, ybar;
    unsigned long long seed;
    const double* xt;             // D x n, feature-major
    const double* y;              // n
    const unsigned short* order;  // D x n: every feature's rows in ascending order of (value, index)
    const int* idx;               // T x n_points bootstrap draws, or nullptr: drawn here
    unsigned short* lists;        // 2 x T x D x n: the per-tree feature lists, ping and pong
    robo_rf_node* nodes;          // T x stride
    int* counts;                  // T
    RfScratch* scr;               // T x stride
};

// the rows' sweep tile: as many candidates per workgroup (a multiple of 64, at most WG) as RF_STAGE_COORDS holds
inline int rf_sweep_tile(int D) {
    const int fit = RF_STAGE_COORDS / (D | 1) / 64 * 64;
    return fit > WG ? WG : fit;
}

int launch_rf_presort(robo_ctx* ctx, const double* d_xt, int n, int D, unsigned short* d_order);
int launch_rf_grow(robo_ctx* ctx, const RfGrow& a);
int launch_rf_sweep(robo_ctx* ctx, const robo_rf_node* d_nodes, const int* d_counts, int stride, int T, int D,
                    int total_variance, const double* d_rows, long long m, double* d_mean, double* d_var,
                    double* d_per_tree);

}  // namespace robo

struct robo_rf {
    robo_ctx* ctx;
    int dim, T;
    int bootstrap, max_features, min_split, min_leaf, max_depth, total_variance;
    double eps_purity;
    bool fitted;
    int stride;                   // nodes per tree in d_nodes
    double* d_data;               // a fit's [Xt (D x n) | y (n)] (grows)
    size_t data_cap;
    unsigned short* d_order;      // D x n, then the lists 2 x T x D x n (grows)
    size_t order_cap;
    robo_rf_node* d_nodes;        // T x stride (grows)
    size_t nodes_cap;
    robo::RfScratch* d_scr;       // T x stride (grows)
    size_t scr_cap;
    int* d_counts;                // T
    int* d_idx;                   // a fit's draws (grows)
    size_t idx_cap;
    double* d_cand;               // the uploaded candidate rows (grows)
    size_t cand_cap;
    double* d_ps;                 // per-tree leaf means (T x m) of a call that asks (grows)
    size_t ps_cap;
    robo_cand* k;                 // the moments' tables and the acquisition's state, kept between calls of one m
};
