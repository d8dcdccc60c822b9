// scale_search_ragged_plan.h -- how a genpc_scale_search_scores_ragged call (scale_search_ragged.hip) treats a pair, decided from
// its source count alone: one workgroup per candidate, the candidate's scaled source and its cell table in a compute unit's
// LDS (scale_search_ragged_kernel), with the cell budget that still fits beside the cloud; or, when the cloud does not fit,
// the existing genpc_scale_search_scores on the pair's slices.  The entry point and the kernel's carve-up of its LDS both
// read this header and decide nothing besides.  The LDS of a workgroup, all of it dynamic (nothing static in front of it):
//   [0, kSsFixed)                       the box reduction's floats | the scan's ints | the score's doubles
//   [kSsFixed, + 16 ns)                 the scaled source in cell order: x, y, z, index
//   [.., + 4 (cells + 1) rounded to 16) first position of every cell, one more for the end
// Host code only, no HIP: a plain C++ program can include it (tests/scale_search_ragged_plan_check.cpp does); the kernel asks
// the plan of its own pair on the device through ragged_offsets.h's GENPC_RAGGED_HD.  The library exports the split of a table
// as genpc_scale_search_ragged_plan.
#pragma once
#include <stddef.h>
#include "ragged_table.h"

namespace genpc {

constexpr int kSsRaggedMaxPairs = 256;                  // three tables of 257 ints = 3084 bytes of the 4096 a kernel may take
constexpr int kSsRaggedMaxPoints = 1 << 28;             // per side, all pairs together
constexpr int kSsRaggedMaxCandidates = 1 << 20;         // all pairs together
constexpr int kSsBlock = 256;                           // threads of a workgroup (cd_score.h's kIBlock: the kernel asserts it)
constexpr int kSsWaves = kSsBlock / 64;
constexpr size_t kSsFixed = (size_t)kSsWaves * 6 * 4 + (size_t)kSsWaves * 2 * 4 + (size_t)kSsWaves * 2 * 8;
constexpr size_t kSsLdsBudget = (size_t)160 * 1024;     // a compute unit's LDS
constexpr size_t kSsLdsReserve = 1024;                  // kept free of it, as icp_plan.h keeps it
constexpr int kSsCellsMin = 1024;                       // the cell budget is halved until cloud and table fit, not below this
constexpr int kSsSourceLimit = 1 << 24;                 // a source of this many points or more is the single call's (it fits no LDS anyway)

GENPC_RAGGED_HD inline size_t scale_search_lds(int ns, int cells)
{
    return kSsFixed + (size_t)ns * 16 + ((size_t)cells + 1 + 3) / 4 * 16;
}

struct ScaleSearchPlan {
    int one_workgroup;      // 1: scale_search_ragged_kernel; 0: genpc_scale_search_scores on the pair alone
    int cells;              // the cell budget of the scaled source's grid (0 for the single call)
    int lds_bytes;          // dynamic LDS of a workgroup (0 for the single call)
};

GENPC_RAGGED_HD inline ScaleSearchPlan scale_search_plan(int ns)
{
    ScaleSearchPlan p{0, 0, 0};
    if (ns <= 0 || ns >= kSsSourceLimit) return p;
    int cells = ragged_cells_max(ns);
    while (scale_search_lds(ns, cells) + kSsLdsReserve > kSsLdsBudget && cells >= 2 * kSsCellsMin) cells >>= 1;
    if (scale_search_lds(ns, cells) + kSsLdsReserve > kSsLdsBudget) return p;
    p.one_workgroup = 1;
    p.cells = cells;
    p.lds_bytes = (int)scale_search_lds(ns, cells);
    return p;
}

// about two points per cell, as ragged_cells_target has it, inside the plan's budget
GENPC_RAGGED_HD inline int scale_search_cells_target(int ns, int cells)
{
    const int t = ragged_cells_target(ns), hi = cells * 3 / 4;
    return t > hi ? hi : t;
}

struct ScaleSearchRaggedPlan {
    int fused_pairs;        // pairs scored by the one launch
    int loop_pairs;         // pairs sent to genpc_scale_search_scores, one after the other
    int lds_bytes;          // dynamic LDS of the one launch: the largest of its pairs' (0 when no pair is in it)
};

// soff[c + 1]: ascending offsets of the pairs' sources (the caller has checked them).  A pair without source points is on
// neither side (it can have no candidates).
inline ScaleSearchRaggedPlan scale_search_ragged_plan(int c, const int *soff)
{
    ScaleSearchRaggedPlan r{0, 0, 0};
    for (int j = 0; j < c; j++) {
        const int ns = soff[j + 1] - soff[j];
        if (ns <= 0) continue;
        const ScaleSearchPlan p = scale_search_plan(ns);
        if (p.one_workgroup) {
            r.fused_pairs++;
            if (p.lds_bytes > r.lds_bytes) r.lds_bytes = p.lds_bytes;
        } else {
            r.loop_pairs++;
        }
    }
    return r;
}

}  // namespace genpc
