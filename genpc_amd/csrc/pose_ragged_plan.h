// pose_ragged_plan.h -- the shape of one ragged alignment call (pose.hip genpc_pose_optimize_ragged, genpc_pose_loss_grad_ragged),
// decided from the scans' sizes alone: how the starts become batch elements, how wide every launch is, which of mask_step_plan's
// choices the silhouette step takes, what the scratch holds, and whether the call is refused for its size.  The two entry
// points branch on nothing but what pose_ragged_plan returns.
// The ragged loop is the SIMPLE form of pose_plan.h's loop: one stream (no side stream, no device-counter hand-over: no kernel
// of the call waits for another), the Adam update a launch of its own (the fused form is for <= 8 elements), nearest neighbours
// from nn_ragged.hip's grid search in both directions (the MFMA filter, the seeded search and the duplicate masks need equal
// sizes) or, where the calling thread asks for it, from nn_ragged_dense.hip's all-pairs search (nn_dense: the same bits).  What it shares with pose_loop_plan -- pose_grad riding in the silhouette gradient's launch, pose_grad's block cap,
// the widths of the one-thread-per-element kernels -- it asks of pose_loop_plan, for `elements` clouds of the largest sizes.
// Element e = scan * starts + start owns starts-fold replicated points: its complete cloud lies at starts * coff[scan] +
// start * nc_scan of the packed element arrays (partial alike), so the element tables ascend and are valid RaggedTables.
// Launch grids are (width for the largest element, elements); a block with nothing to do in a short element leaves.
// Host code only, no HIP: a plain C++ program can include it (tests/pose_ragged_plan_check.cpp does, under the sanitizers); the
// library exports the plan as genpc_pose_ragged_plan.
#pragma once
#include "pose_plan.h"
#include "ragged_table.h"

namespace genpc {

struct PoseRaggedAsk {
    int c = 0;                        // scans
    const int *coff = nullptr;        // c + 1 ascending offsets of the complete clouds (the caller has checked them: no empty cloud)
    const int *poff = nullptr;        // ... of the partial clouds
    int starts = 1;                   // multi-starts per scan, side by side as batch elements
    bool mask = false;                // the full objective
    int render_size = 0;
    float radius = 0.0f;
    int cus = 256;                    // compute units of the device (reported only: no width depends on it)
    int nn_dense = 0;                 // the calling thread's ragged search (genpc_nn_ragged_tune): 0 the grid search, 1 all pairs
};

struct PoseRaggedPlan {
    int elements;                     // scans x starts
    int nc_max, np_max;               // the largest complete / partial cloud: the launches' widths are for these
    long long total_c, total_p;       // points of the packed ELEMENT arrays (starts-fold): sizes pts, d1 / i1, d2 / i2, uvr, zex
    bool replicate;                   // starts > 1: the clouds are copied once per start at the head of the call
    const char *too_large;            // null, or why the call is refused
    int g_t;                          // blocks per element of the transform (and of the projections)
    int g_g;                          // ... of pose_grad
    int gb;                           // blocks of the one-thread-per-element kernels
    int g_m;                          // blocks per element of the centre's sums
    int g_rep;                        // blocks per scan of the replication
    bool ride;                        // pose_grad's blocks in the silhouette gradient's launch
    MaskStepPlan step;                // gp, gs as mask_step_plan has them; fuse_w and sub8 from the totals (the mean element)
    int nmax_piece;                   // per-element count that sizes MaskScratch's uvr / zex: elements x this >= both totals
    int blocks_per_cu;                // the transform launch's blocks per compute unit, rounded up (a figure, not a decision)
    int nn_dense;                     // nearest neighbours by all pairs (nn_ragged_dense.hip): two launches a step, no grid built or kept
};

// element tables of a call: e = scan * starts + start
inline void pose_ragged_element_offsets(int c, const int *off, int starts, int *off_e /* c * starts + 1 */)
{
    for (int j = 0; j < c; j++) {
        const int n = off[j + 1] - off[j];
        for (int s = 0; s < starts; s++) off_e[j * starts + s] = starts * off[j] + s * n;
    }
    off_e[c * starts] = starts * off[c];
}

inline PoseRaggedPlan pose_ragged_plan(const PoseRaggedAsk &a)
{
    PoseRaggedPlan p{};
    const long long elements = (long long)a.c * a.starts;
    if (elements > kRaggedMaxPairs) {
        p.too_large = "more than 384 elements (scans x starts) in one call";
        return p;
    }
    p.elements = (int)elements;
    for (int j = 0; j < a.c; j++) {
        p.nc_max = std::max(p.nc_max, a.coff[j + 1] - a.coff[j]);
        p.np_max = std::max(p.np_max, a.poff[j + 1] - a.poff[j]);
    }
    p.total_c = a.c > 0 ? (long long)a.starts * a.coff[a.c] : 0;
    p.total_p = a.c > 0 ? (long long)a.starts * a.poff[a.c] : 0;
    if (p.total_c > kRaggedMaxPoints || p.total_p > kRaggedMaxPoints) {
        p.too_large = "more than 2^28 points on one side (scans x starts)";
        return p;
    }
    p.replicate = a.starts > 1;
    p.nn_dense = a.nn_dense != 0;
    if (p.elements == 0) return p;

    // what the equal-size loop decides for `elements` clouds on one stream: taken over, not restated
    PoseLoopAsk la;
    la.scans = p.elements; la.starts = 1; la.nc = p.nc_max; la.np = p.np_max; la.mask = a.mask;
    la.side_stream_ok = false; la.counters_ok = false;
    const PoseLoopPlan lp = pose_loop_plan(la);
    p.g_t = lp.g_t;
    p.g_g = lp.g_g;
    p.gb = lp.gb;
    p.ride = lp.ride;
    p.g_m = lin_grid(p.nc_max);
    p.g_rep = lin_grid(3ll * std::max(p.nc_max, p.np_max));
    // the silhouette step: how many points gather and how many lanes share one is a matter of the work in flight -- the totals,
    // i.e. the mean element -- not of the largest element (a call of one size: mask_step_plan of that size)
    const int nc_mean = (int)((p.total_c + p.elements - 1) / p.elements);
    if (a.mask) p.step = mask_step_plan(p.elements, nc_mean, a.render_size, a.radius);
    const long long most = std::max(p.total_c, p.total_p);
    p.nmax_piece = (int)((most + p.elements - 1) / p.elements);
    const long long cus = a.cus > 0 ? a.cus : 1;
    p.blocks_per_cu = (int)(((long long)p.g_t * p.elements + cus - 1) / cus);
    return p;
}

}  // namespace genpc
