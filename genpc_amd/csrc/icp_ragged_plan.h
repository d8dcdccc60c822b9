// icp_ragged_plan.h -- how a genpc_icp_batch_ragged call (icp.hip) is split, decided from the pairs' target counts alone: the
// pairs whose target gets icp_plan.h's one-workgroup plan are all solved by ONE launch (icp_fused_ragged_kernel: a workgroup per
// (pair, candidate), each carving its LDS by its own pair's plan), whose dynamic LDS is the largest of their plans'; the others
// are solved one after the other by genpc_icp_batch's multi-launch loop.  A pair without targets is on neither side (it can
// have no candidates).  genpc_icp_batch_ragged reads this header and decides nothing besides.
// Host code only, no HIP: a plain C++ program can include it (tests/icp_ragged_plan_check.cpp does); the library exports the
// function as genpc_icp_ragged_plan.
#pragma once
#include "icp_plan.h"

namespace genpc {

constexpr int kIcpRaggedMaxPairs = 256;       // three tables of 257 ints = 3084 bytes of the 4096 a kernel may take
constexpr int kIcpRaggedMaxPoints = 1 << 28; // per side, all pairs together
constexpr int kIcpRaggedMaxCandidates = 1 << 20;      // all pairs together

struct IcpRaggedPlan {
    int fused_pairs;        // pairs solved by the one launch
    int loop_pairs;         // pairs sent to the multi-launch loop, one after the other
    int lds_bytes;          // dynamic LDS of the one launch (0 when no pair is in it)
};

// toff[c + 1]: ascending offsets of the pairs' targets (the caller has checked them)
inline IcpRaggedPlan icp_ragged_plan(int c, const int *toff)
{
    IcpRaggedPlan r{0, 0, 0};
    for (int j = 0; j < c; j++) {
        const int nt = toff[j + 1] - toff[j];
        if (nt <= 0) continue;
        const IcpPlan p = icp_plan(nt);
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
