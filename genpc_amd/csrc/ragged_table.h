// ragged_table.h -- the pair table of a ragged call (nn_ragged.hip, grid.hip's ragged build): which slice of the packed
// queries and of the packed targets belongs to pair j.  It travels BY VALUE in the kernel arguments of both launches: no
// copy is enqueued, nothing of the caller's arrays is looked at after the entry point returns, and a captured graph holds
// the table itself.  That is what bounds the number of pairs (kernel arguments are 4 KiB); every index a kernel forms into
// it is uniform over the workgroup, so the reads are scalar loads of the argument segment.
// Nothing here needs a prefix sum on the device: where pair j's pieces lie follows from its own two offsets and j.
//   * its cell table (first sorted position of every cell, one more for the end) starts at toff[j] + 65 j of `start` and
//     has room for ragged_cells_max(m_j) + 1 = at most m_j + 65 entries;
//   * its queries are dealt to workgroups of 64 lanes, the first of them numbered (qoff[j] >> 6) + j; pair j needs
//     ceil(n_j / 64) <= (qoff[j + 1] >> 6) - (qoff[j] >> 6) + 1 of them, so the ranges do not overlap, the numbering ascends
//     strictly (a binary search finds the pair of a workgroup) and at most one workgroup per pair finds nothing to do.
// The check of the offsets, the padded copy and the search itself are ragged_offsets.h's.
// Host code only, no HIP: a plain C++ program can include it (tests/ragged_table_check.cpp does, under the sanitizers).
#pragma once
#include "ragged_offsets.h"

namespace genpc {

constexpr int kRaggedMaxPairs = 384;              // 2 x 385 ints = 3080 bytes of the 4096 a kernel may take
constexpr int kRaggedMaxPoints = 1 << 28;         // per side, all pairs together: positions, 65 c more and 3 x either stay ints / size_t
constexpr int kRaggedCellsCap = 15360;            // = kCellGridMaxCells (grid.h asserts it)
constexpr int kRaggedStartPad = 65;               // cell-table entries of a pair beyond its m_j
constexpr int kRaggedLanes = 64;                  // queries per workgroup of the search

struct RaggedTable {
    int c;
    int qoff[kRaggedMaxPairs + 1];                // queries of pair j: [qoff[j], qoff[j + 1])
    int toff[kRaggedMaxPairs + 1];                // targets of pair j: [toff[j], toff[j + 1])
};

// cells a pair's grid may have: no more than its targets (and a few, for the smallest), nor than the build's LDS counters
GENPC_RAGGED_HD inline int ragged_cells_max(int m) { return m + kRaggedStartPad - 1 < kRaggedCellsCap ? m + kRaggedStartPad - 1 : kRaggedCellsCap; }
// about two targets per cell, as the k-nearest search sizes its grid for k <= 5
GENPC_RAGGED_HD inline int ragged_cells_target(int m)
{
    const int t = m / 2, hi = ragged_cells_max(m) * 3 / 4;
    return t < 8 ? 8 : (t > hi ? hi : t);
}
inline long long ragged_start_len(long long targets, int c) { return targets + (long long)kRaggedStartPad * c; }
inline long long ragged_items(long long queries, int c) { return (queries >> 6) + c; }

// Checks the caller's offsets and copies them.  1: there is work; 0: nothing to do (no pair, or no query in any); -1 with
// *err set: refused.  *max_targets: the largest target cloud among the pairs that have queries.
inline int ragged_table_fill(int c, const int *noff, const int *moff, RaggedTable &t, int *max_targets, const char **err)
{
    *err = nullptr;
    *max_targets = 0;
    if (c < 0) { *err = "negative number of pairs"; return -1; }
    if (c == 0) return 0;
    if (!noff || !moff) { *err = "null offset table"; return -1; }
    if (c > kRaggedMaxPairs) { *err = "more than 384 pairs in one call"; return -1; }
    if ((*err = ragged_offsets_fault(c, {noff, moff}))) return -1;
    if (noff[c] > kRaggedMaxPoints || moff[c] > kRaggedMaxPoints) { *err = "more than 2^28 points on one side"; return -1; }
    if (noff[c] == 0) return 0;
    for (int j = 0; j < c; j++) {
        const int n = noff[j + 1] - noff[j], m = moff[j + 1] - moff[j];
        if (n > 0 && m == 0) { *err = "a pair has queries and no targets"; return -1; }
        if (n > 0 && m > *max_targets) *max_targets = m;
    }
    t.c = c;
    ragged_pad_copy(t.qoff, noff, c);
    ragged_pad_copy(t.toff, moff, c);
    return 1;
}

// the pair a workgroup of the search serves: the largest j with (qoff[j] >> 6) + j <= item   (0 <= item < ragged_items)
GENPC_RAGGED_HD inline int ragged_pair_of(const RaggedTable &t, int item) { return ragged_item_owner(t.qoff, t.c, item, 6); }

}  // namespace genpc
