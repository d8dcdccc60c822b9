// icp_plan.h -- which implementation a genpc_icp_batch call runs (icp.hip), decided from the target count alone: the
// one-workgroup solve (icp_fused_kernel: one launch, the target cloud and its grid in a compute unit's LDS) with the cell
// budget that still fits beside the cloud, or the multi-launch loop (five launches per pass).  genpc_icp_batch and the
// kernel's carve-up of its LDS read this header and decide nothing besides.
// Host code only, no HIP: a plain C++ program can include it (tests/icp_plan_check.cpp does); the library exports the
// function as genpc_icp_plan, and the GPU tests take their sizes from that call.
#pragma once
#include <stddef.h>

// icp.hip defines this as ragged_offsets.h's GENPC_RAGGED_HD before it includes the header: the one-launch kernel of
// genpc_icp_batch_ragged asks the plan of its own pair on the device.  Everywhere else it is nothing, and the header plain C++.
#ifndef GENPC_ICP_PLAN_HD
#define GENPC_ICP_PLAN_HD
#endif

namespace genpc {

constexpr int kFT = 1024;                    // threads of the one-workgroup solve
constexpr int kFWaves = kFT / 64;            // its waves (64 lanes: icp.hip asserts this against kWave)
constexpr int kFItems = 512;                 // (query, neighbour cell) pairs of one wave per round of the list
// what the kernel keeps in LDS beside the cloud and the cells: per thread a query (float4) and its best key (8 bytes), per wave
// the pair list, the 17 sums per wave, the transform, the sums
constexpr size_t kFFixed = (size_t)kFT * 16 + (size_t)kFT * 8 + (size_t)kFWaves * kFItems * 4 + (size_t)17 * kFWaves * 8 + 16 * 8 + 17 * 8;
constexpr size_t kFLdsBudget = (size_t)160 * 1024;      // a compute unit's LDS
constexpr size_t kFLdsStatic = 1024;                    // room for the kernel's __shared__ variables (frame, state, scan scratch)
constexpr int kFCellsMax = 8192, kFCellsMin = 1024;     // the grid's cell budget: halved until cloud and grid fit
constexpr int kFIndexLimit = 65536;                     // a key holds the target's position in 16 bits

// LDS of the one-workgroup solve for nt targets with `cells` grid cells: the cloud as float4, padded to a multiple of four
GENPC_ICP_PLAN_HD inline size_t icp_fused_lds(int nt, int cells) { return ((size_t)nt + 3) / 4 * 4 * 16 + (size_t)cells * 4 + kFFixed; }

struct IcpPlan {
    int one_workgroup;      // 1: icp_fused_kernel, one launch per call; 0: the multi-launch loop
    int cells;              // the grid's cell budget (0 for the loop)
    int lds_bytes;          // dynamic LDS of the launch (0 for the loop)
};

GENPC_ICP_PLAN_HD inline IcpPlan icp_plan(int nt)
{
    IcpPlan p{0, 0, 0};
    if (nt <= 0 || nt >= kFIndexLimit) return p;
    int cells = kFCellsMax;
    while (cells >= kFCellsMin && icp_fused_lds(nt, cells) + kFLdsStatic > kFLdsBudget) cells >>= 1;
    if (cells < kFCellsMin) return p;
    p.one_workgroup = 1;
    p.cells = cells;
    p.lds_bytes = (int)icp_fused_lds(nt, cells);
    return p;
}

}  // namespace genpc
