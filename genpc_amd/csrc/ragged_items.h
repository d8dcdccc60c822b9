// ragged_items.h -- ragged_table.h's numbering of a launch's workgroups, for workgroups that own 2^shift queries instead of 64.
//
// Pair j's queries [qoff[j], qoff[j + 1]) are dealt to work items of 2^shift queries; its first item is numbered
// (qoff[j] >> shift) + j.  With a = qoff[j], b = qoff[j + 1] and K = 2^shift the pair needs
//     ceil((b - a) / K)  <=  floor(b / K) - floor(a / K) + 1
// items (write a = K a' + r, b = K b' + s with 0 <= r, s < K: b - a = K (b' - a') + s - r <= K (b' - a') + K - 1, whose
// ceiling over K is at most b' - a' + 1), and the right-hand side is the distance to pair j + 1's first item.  So: the
// ranges do not overlap, the numbering ascends strictly (every pair owns at least the item of its own `+ j`), a binary
// search finds the pair of an item, an item's queries never leave its pair, and at most one item per pair -- the last of its
// range -- finds nothing to do.  shift = 6 is ragged_table.h's own numbering (ragged_items, ragged_pair_of); shift = 10 serves
// the 1024 queries a workgroup of uhd_ragged.hip owns.
// Host code only, no HIP: tests/uhd_ragged_table_check.cpp includes it under the sanitizers.
#pragma once
#include "ragged_table.h"

namespace genpc {

// the number of the first work item of pair j   (0 <= j <= c; j == c: the number of items of the launch)
GENPC_RAGGED_HD inline int ragged_first_item_shift(const RaggedTable &t, int j, int shift) { return (t.qoff[j] >> shift) + j; }
inline long long ragged_items_shift(long long queries, int c, int shift) { return (queries >> shift) + c; }

// the pair a work item serves: the largest j with (qoff[j] >> shift) + j <= item   (0 <= item < ragged_items_shift)
GENPC_RAGGED_HD inline int ragged_pair_of_shift(const RaggedTable &t, int item, int shift) { return ragged_item_owner(t.qoff, t.c, item, shift); }

// the first query of a work item, counted inside its pair; at or beyond the pair's size: the item is idle
GENPC_RAGGED_HD inline long long ragged_item_base_shift(const RaggedTable &t, int pair, int item, int shift)
{
    return (long long)(item - ragged_first_item_shift(t, pair, shift)) << shift;
}

}  // namespace genpc
