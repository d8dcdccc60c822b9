// nn_ragged_dense_plan.h -- the shape of one all-pairs ragged nearest-neighbour call (nn_ragged_dense.hip), decided from the pair
// table alone: how many work items, how a workgroup is cut into queries and into target tiles, what LDS it takes, how many pair
// evaluations the call is, and whether it is refused for its size.  The launcher and the kernel read the constants and the plan
// and decide nothing besides.
//   * an item is kNnDenseQueries = 64 queries of one pair in nn_ragged_kernel's numbering (ragged_items, ragged_pair_of);
//   * its workgroup is kNnDenseThreads = 256 threads, four waves on the same 64 queries; the pair's targets pass through LDS in
//     tiles of kNnDenseTile, of which wave w scans [w kNnDenseShare, (w + 1) kNnDenseShare);
//   * the LDS of a workgroup: the tile as float4 (the four waves' results are combined through its head once the last tile is
//     scanned) and one flag word per wave.
// The two refusals keep a call from holding a shared GPU for long; they are conditions, not measurements:
//   * more than 2^36 pair evaluations (sum of n_j m_j): about 16 ms at the chip's fp32 VALU peak at nine instructions a pair;
//   * a pair with queries and more than 2^20 targets: one workgroup walks all of its pair's targets, about 10^7 cycles there.
// Host code only, no HIP: a plain C++ program can include it (tests/nn_ragged_dense_plan_check.cpp does, under the sanitizers);
// the library exports the plan as genpc_nn_ragged_dense_plan.
#pragma once
#include <stddef.h>
#include "ragged_table.h"

namespace genpc {

constexpr int kNnDenseThreads = 256;                              // threads of a workgroup
constexpr int kNnDenseWaves = kNnDenseThreads / 64;
constexpr int kNnDenseQueries = kRaggedLanes;                     // queries of an item: one per lane, the same in every wave
constexpr int kNnDenseTile = 1024;                                // targets staged at a time
constexpr int kNnDenseShare = kNnDenseTile / kNnDenseWaves;       // ... of which a wave scans this many
constexpr int kNnDenseLoads = kNnDenseTile * 3 / kNnDenseThreads; // floats a thread fetches per tile
constexpr size_t kNnDenseLds = (size_t)kNnDenseTile * 16 + (size_t)kNnDenseWaves * 4;
constexpr size_t kNnDenseLdsLimit = (size_t)64 * 1024;            // what a workgroup may take of a compute unit's LDS without asking
constexpr long long kNnDenseMaxEvals = 1ll << 36;                 // pair evaluations of one call
constexpr int kNnDenseMaxTargets = 1 << 20;                       // targets of one pair

static_assert(kNnDenseTile % kNnDenseWaves == 0 && (kNnDenseTile * 3) % kNnDenseThreads == 0, "a tile is dealt out evenly");
static_assert((size_t)(kNnDenseWaves - 1) * kNnDenseQueries * 8 <= (size_t)kNnDenseTile * 16, "the combine fits the tile's LDS");
static_assert(kNnDenseLds <= kNnDenseLdsLimit, "a workgroup's LDS");

struct NnRaggedDensePlan {
    long long items;                  // workgroups of the launch
    int threads;                      // per workgroup
    int queries;                      // per item
    int tile;                         // targets per tile
    int share;                        // targets per wave's share of a tile
    int lds_bytes;
    long long evals;                  // sum over the pairs of n_j m_j
    const char *too_large;            // null, or why the call is refused
};

inline NnRaggedDensePlan nn_ragged_dense_plan(const RaggedTable &t)
{
    NnRaggedDensePlan p{};
    p.items = ragged_items(t.qoff[t.c], t.c);
    p.threads = kNnDenseThreads;
    p.queries = kNnDenseQueries;
    p.tile = kNnDenseTile;
    p.share = kNnDenseShare;
    p.lds_bytes = (int)kNnDenseLds;
    for (int j = 0; j < t.c; j++) {
        const long long n = t.qoff[j + 1] - t.qoff[j], m = t.toff[j + 1] - t.toff[j];
        if (n > 0 && m > kNnDenseMaxTargets && !p.too_large) p.too_large = "the dense search takes at most 2^20 targets in a pair";
        p.evals += n * m;             // (at most 2^28 x 2^28 in all: no overflow)
    }
    if (p.evals > kNnDenseMaxEvals && !p.too_large) p.too_large = "the dense search takes at most 2^36 pair evaluations in a call";
    return p;
}

}  // namespace genpc
