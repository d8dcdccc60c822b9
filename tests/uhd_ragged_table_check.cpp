// uhd_ragged_table_check.cpp -- csrc/ragged_items.h as a plain host program (tests/test_uhd_ragged_host.py builds it with the
// address and undefined-behaviour sanitizers): the numbering of work items of 2^shift queries that uhd_ragged.hip's workgroups
// find their pair and their queries by.  For every table of the sweep and for shift 10 (and 6, which must restate
// ragged_table.h's own numbering): the first items ascend strictly, the ranges do not overlap and hold the items a pair needs,
// the search names the right pair for every item, at most one item per pair is idle, and no query index leaves its pair.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "ragged_items.h"

using namespace genpc;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static long long tables = 0;

static void check(const std::vector<int> &sizes, int shift)
{
    const int c = (int)sizes.size();
    std::vector<int> n((size_t)c + 1, 0), m((size_t)c + 1, 0);
    for (int j = 0; j < c; j++) {
        n[(size_t)j + 1] = n[(size_t)j] + sizes[(size_t)j];
        m[(size_t)j + 1] = m[(size_t)j] + 1 + j % 3;
    }
    RaggedTable t;
    int mx = 0;
    const char *err = nullptr;
    EXPECT(ragged_table_fill(c, n.data(), m.data(), t, &mx, &err) == 1 && !err);
    if (err) return;
    tables++;
    const long long K = 1ll << shift, items = ragged_items_shift(t.qoff[c], c, shift);
    EXPECT(ragged_first_item_shift(t, 0, shift) == 0 && ragged_first_item_shift(t, c, shift) == items);
    std::vector<int> owner((size_t)items, -1);
    std::vector<char> seen((size_t)t.qoff[c], 0);
    for (int j = 0; j < c; j++) {
        const long long size = sizes[(size_t)j], first = ragged_first_item_shift(t, j, shift), next = ragged_first_item_shift(t, j + 1, shift);
        const long long need = (size + K - 1) / K;
        EXPECT(first < next);                                   // ascends strictly: every pair owns an item
        EXPECT(first + need <= next);                           // room for the pair's queries before the next pair's first item
        EXPECT(next - first - need <= 1);                       // at most one idle item
        int idle = 0;
        for (long long w = first; w < next; w++) {
            EXPECT(owner[(size_t)w] == -1);                     // ranges never overlap
            owner[(size_t)w] = j;
            EXPECT(ragged_pair_of_shift(t, (int)w, shift) == j);
            if (shift == 6) EXPECT(ragged_pair_of(t, (int)w) == j);
            const long long base = ragged_item_base_shift(t, j, (int)w, shift);
            EXPECT(base == (w - first) * K && base >= 0);
            if (base >= size) { idle++; continue; }             // the kernels' test for "nothing to do"
            for (long long i = base; i < base + K && i < size; i++) {
                const long long at = (long long)t.qoff[j] + i;  // no query index leaves its pair
                EXPECT(at >= t.qoff[j] && at < t.qoff[j + 1]);
                EXPECT(!seen[(size_t)at]);
                seen[(size_t)at] = 1;
            }
        }
        EXPECT(idle <= 1);
    }
    for (long long w = 0; w < items; w++) EXPECT(owner[(size_t)w] >= 0);
    for (long long i = 0; i < t.qoff[c]; i++) EXPECT(seen[(size_t)i]);          // and every query is served once
    if (shift == 6) EXPECT(items == ragged_items(t.qoff[c], c));
}

int main()
{
    const int sizes[] = {1, 1023, 1024, 1025, 2049};
    for (int shift : {10, 6}) {
        // c = 1: every size alone
        for (int a : sizes) check({a}, shift);
        check({5000}, shift);
        // pairs and triples of every combination: boundaries fall at 1, 1023, 1024, 1025, 2047, 2048, 2049, 2050, 3072 .. --
        // aligned to 1024, one off either way, and far from it
        for (int a : sizes)
            for (int b : sizes) {
                check({a, b}, shift);
                for (int d : sizes) check({a, b, d}, shift);
            }
        // a multiple of 1024 at an unaligned offset, and the same behind an aligned one
        check({7, 2048, 3}, shift);
        check({1024, 2048, 1}, shift);
        // c = 384: all ones (every boundary inside the first item's range), the five sizes in turn, and pseudo-random sizes
        check(std::vector<int>((size_t)kRaggedMaxPairs, 1), shift);
        {
            std::vector<int> v((size_t)kRaggedMaxPairs);
            for (int j = 0; j < kRaggedMaxPairs; j++) v[(size_t)j] = sizes[j % 5];
            check(v, shift);
            unsigned s = 4242u;
            for (int rep = 0; rep < 20; rep++) {
                const int c = rep < 10 ? kRaggedMaxPairs : 1 + (int)((s = s * 1664525u + 1013904223u) >> 8) % kRaggedMaxPairs;
                v.assign((size_t)c, 0);
                for (int j = 0; j < c; j++) v[(size_t)j] = 1 + (int)((s = s * 1664525u + 1013904223u) >> 8) % 3000;
                check(v, shift);
            }
        }
    }
    // the largest totals: 384 pairs sharing 2^28 queries (the first items must still fit an int and ascend)
    {
        RaggedTable t;
        std::vector<int> n((size_t)kRaggedMaxPairs + 1), m((size_t)kRaggedMaxPairs + 1);
        for (int j = 0; j <= kRaggedMaxPairs; j++) {
            n[(size_t)j] = (int)((long long)kRaggedMaxPoints * j / kRaggedMaxPairs);
            m[(size_t)j] = j;
        }
        int mx = 0;
        const char *err = nullptr;
        EXPECT(ragged_table_fill(kRaggedMaxPairs, n.data(), m.data(), t, &mx, &err) == 1);
        const long long items = ragged_items_shift(t.qoff[t.c], t.c, 10);
        EXPECT(items == (kRaggedMaxPoints >> 10) + kRaggedMaxPairs);
        for (int j = 0; j < t.c; j++) {
            const long long first = ragged_first_item_shift(t, j, 10), next = ragged_first_item_shift(t, j + 1, 10);
            const long long need = ((long long)n[(size_t)j + 1] - n[(size_t)j] + 1023) / 1024;
            EXPECT(first < next && first + need <= next && next - first - need <= 1);
            EXPECT(ragged_pair_of_shift(t, (int)first, 10) == j && ragged_pair_of_shift(t, (int)next - 1, 10) == j);
        }
    }
    if (fails) return 1;
    printf("uhd_ragged_table_check: ok (%lld tables)\n", tables);
    return 0;
}
