// ragged_cand.h -- the table of a ragged call whose pairs bring candidates (genpc_icp_batch_ragged: initial transforms;
// genpc_scale_search_scores_ragged: scales): where pair j's source, target and candidates lie in the packed arrays.  It travels
// BY VALUE at the head of the kernel arguments, as ragged_table.h's does; one workgroup serves one candidate and finds its pair
// by ragged_offsets.h's search over koff (uniform: scalar loads), which passes over the pairs without candidates.
// What both entry points refuse about the table is decided here, in one order.
// Host code only, no HIP: tests/ragged_offsets_check.cpp includes it under the sanitizers.
#pragma once
#include <stdio.h>
#include "ragged_offsets.h"

namespace genpc {

constexpr int kRaggedCandMaxPairs = 256;              // three tables of 257 ints = 3084 bytes of the 4096 a kernel may take
constexpr int kRaggedCandMaxPoints = 1 << 28;         // per side, all pairs together
constexpr int kRaggedCandMaxCandidates = 1 << 20;     // all pairs together

struct RaggedCandTable {
    int c;
    int soff[kRaggedCandMaxPairs + 1];         // source of pair j: [soff[j], soff[j + 1])
    int toff[kRaggedCandMaxPairs + 1];         // its target
    int koff[kRaggedCandMaxPairs + 1];         // its candidates
};

inline void ragged_cand_fill(RaggedCandTable &t, int c, const int *soff, const int *toff, const int *koff)
{
    t.c = c;
    ragged_pad_copy(t.soff, soff, c);
    ragged_pad_copy(t.toff, toff, c);
    ragged_pad_copy(t.koff, koff, c);
}

// the pair of candidate `cand` (0 <= cand < koff[c])
GENPC_RAGGED_HD inline int ragged_cand_pair_of(const RaggedCandTable &t, int cand) { return ragged_owner(t.koff, t.c, cand); }

// The number of pairs.  1: go on; 0: no pair, nothing to do; -1 with *what set: refused.
inline int ragged_cand_count(int c, const char **what)
{
    if (c < 0) { *what = "negative number of pairs"; return -1; }
    if (c == 0) return 0;
    if (c > kRaggedCandMaxPairs) { *what = "more than 256 pairs in one call"; return -1; }
    static_assert(kRaggedCandMaxPairs == 256, "the message above names the bound");
    return 1;
}

// The whole table.  1: there are candidates; 0: none, nothing to do; -1 with *what set (a literal, or text in buf): refused.
inline int ragged_cand_check(int c, const int *soff, const int *toff, const int *koff, const char **what, char (&buf)[96])
{
    const int some = ragged_cand_count(c, what);
    if (some <= 0) return some;
    if (!soff || !toff || !koff) { *what = "null offset table"; return -1; }
    for (const int *off : {soff, toff, koff})
        if ((*what = ragged_offsets_fault(c, off))) return -1;
    if (soff[c] > kRaggedCandMaxPoints || toff[c] > kRaggedCandMaxPoints) { *what = "more than 2^28 points on one side"; return -1; }
    if (koff[c] > kRaggedCandMaxCandidates) { *what = "more than 2^20 candidates"; return -1; }
    for (int j = 0; j < c; j++) {
        if (koff[j + 1] == koff[j]) continue;          // a pair without candidates is skipped, whatever its clouds
        if (soff[j + 1] == soff[j] || toff[j + 1] == toff[j]) {
            snprintf(buf, sizeof buf, "pair %d has candidates and an empty %s", j, soff[j + 1] == soff[j] ? "source" : "target");
            *what = buf;
            return -1;
        }
    }
    return koff[c] > 0 ? 1 : 0;
}

}  // namespace genpc
