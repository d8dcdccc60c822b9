// emd_ragged_plan.h -- the launch plan of the ragged auction's bid kernel (emd_ragged.hip) as a pure function of the pairs'
// offsets and a CU count: how many workgroups each pair owns, their prefix, the grid, and the workgroup -> (pair,
// workgroup-in-pair) lookup the kernel uses.  The table travels BY VALUE in the kernel arguments like ragged_table.h's.
//   * A pair's run of workgroups is fixed for the whole call and sized from N_j alone: its share of ~16 workgroups per CU
//     in proportion to its points (the dense bid's occupancy target, emd.hip), at least 1, at most kEmdRaggedMaxBlocks,
//     and never more than the finest split needs -- 64 lanes per bidder, all N_j bidding: ceil(N_j * 64 / 256).
//   * An empty pair owns no workgroup: first[j] == first[j + 1].  The lookup is the largest j with first[j] <= block, which
//     skips empty pairs whether they lie before, between or behind the others.
//   * The grid is at most 384 * 1024 workgroups: far below 2^31.
// Host code only, no HIP: tests/emd_ragged_plan_check.cpp includes it under the sanitizers.
#pragma once
#include "ragged_offsets.h"

namespace genpc {

constexpr int kEmdRaggedMaxPairs = 384;           // = kRaggedMaxPairs: 2 x 385 ints of the 4096 bytes a kernel may take
constexpr int kEmdRaggedBlock = 256;              // = kEBlock (emd.h), threads of a bid workgroup
constexpr int kEmdRaggedMaxBlocks = 1024;         // per pair: more only add dispatch latency (emd.hip measured it for one cloud)
constexpr int kEmdRaggedBlocksPerCu = 16;         // the whole launch aims at this many workgroups per CU

struct EmdRaggedTable {
    int c;
    int off[kEmdRaggedMaxPairs + 1];              // points AND objects of pair j: [off[j], off[j + 1])
    int first[kEmdRaggedMaxPairs + 1];            // bid workgroups of pair j: [first[j], first[j + 1]); first[c] is the grid
};

// the most workgroups pair of n points can use: one bidder per wave, everybody bidding
GENPC_RAGGED_HD inline int emd_ragged_block_cap(int n)
{
    const long long cap = ((long long)n * 64 + kEmdRaggedBlock - 1) / kEmdRaggedBlock;
    return cap > kEmdRaggedMaxBlocks ? kEmdRaggedMaxBlocks : (int)cap;
}

// workgroups of a pair of n points in a call of `total` points on `cus` compute units
inline int emd_ragged_blocks_of(int n, long long total, int cus)
{
    if (n <= 0) return 0;
    if (cus < 1) cus = 1;
    const long long want = (long long)cus * kEmdRaggedBlocksPerCu;
    long long g = (want * n + total - 1) / total;           // total >= n > 0
    const int cap = emd_ragged_block_cap(n);
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

// Fills t from c + 1 checked offsets (ascending from 0, c <= kEmdRaggedMaxPairs); returns the grid.
inline int emd_ragged_plan(int c, const int *off, int cus, EmdRaggedTable &t)
{
    t.c = c;
    const long long total = off[c];
    int at = 0;
    ragged_pad_copy(t.off, off, c);
    for (int j = 0; j < c; j++) {
        t.first[j] = at;
        at += emd_ragged_blocks_of(off[j + 1] - off[j], total, cus);
    }
    for (int j = c; j <= kEmdRaggedMaxPairs; j++) t.first[j] = at;
    return at;
}

// the pair that owns workgroup `block` of the bid launch (0 <= block < first[c]): the largest j with first[j] <= block
GENPC_RAGGED_HD inline int emd_ragged_pair_of_block(const EmdRaggedTable &t, int block) { return ragged_owner(t.first, t.c, block); }

// the pair that owns point (or object) `pos` of the packed arrays (0 <= pos < off[c]): the largest j with off[j] <= pos
GENPC_RAGGED_HD inline int emd_ragged_pair_of_point(const EmdRaggedTable &t, int pos) { return ragged_owner(t.off, t.c, pos); }

}  // namespace genpc
