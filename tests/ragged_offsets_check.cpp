// ragged_offsets_check.cpp -- csrc/ragged_offsets.h and csrc/ragged_cand.h as a plain host program (tests/test_ragged_offsets.py
// builds it with the address and undefined-behaviour sanitizers): the offset check, the padded copy, the two searches against a
// linear scan over EVERY valid argument, the work-item numbering ragged_items.h claims, and the refusals the ICP and scale
// search entry points share, in their order.
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "ragged_cand.h"

using namespace genpc;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static std::vector<int> offsets(const std::vector<int> &sizes)
{
    std::vector<int> off(1, 0);
    for (int n : sizes) off.push_back(off.back() + n);
    return off;
}

// ragged_owner over every packed position, against the definition: position x belongs to the one j with off[j] <= x < off[j + 1]
static void check_owner(const std::vector<int> &off)
{
    const int c = (int)off.size() - 1;
    for (int j = 0; j < c; j++)
        for (int x = off[(size_t)j]; x < off[(size_t)j + 1]; x++) {
            const int got = ragged_owner(off.data(), c, x);
            if (got != j) { printf("FAILED ragged_owner: c %d x %d -> %d, not %d\n", c, x, got, j); fails++; return; }
        }
}

// ragged_item_owner over every work item, against a linear scan; and the numbering itself: pair j's items start at
// (off[j] >> shift) + j, it needs ceil(n_j / 2^shift) of them, and the next pair's first item lies beyond the last it needs
static void check_items(const std::vector<int> &off, int shift)
{
    const int c = (int)off.size() - 1;
    auto first = [&](int j) { return (off[(size_t)j] >> shift) + j; };
    const int items = first(c);
    std::vector<int> owner((size_t)items, -1);
    for (int j = 0; j < c; j++) {
        const int n = off[(size_t)j + 1] - off[(size_t)j], need = (n + (1 << shift) - 1) >> shift;
        EXPECT(first(j) + need <= first(j + 1));                  // the ranges do not overlap
        EXPECT(first(j) < first(j + 1));                          // every pair owns at least the item of its own `+ j`
        EXPECT(first(j + 1) - first(j) - need <= 1);              // at most one idle item per pair
        for (int w = first(j); w < first(j + 1); w++) {
            EXPECT(owner[(size_t)w] == -1);
            owner[(size_t)w] = j;
        }
    }
    for (int w = 0; w < items; w++) {
        int scan = 0;
        for (int j = 0; j < c; j++)
            if (first(j) <= w) scan = j;
        const int got = ragged_item_owner(off.data(), c, w, shift);
        if (got != scan || owner[(size_t)w] != scan) {
            printf("FAILED ragged_item_owner: c %d shift %d item %d -> %d, scan %d, range %d\n", c, shift, w, got, scan, owner[(size_t)w]);
            fails++;
            return;
        }
    }
}

static void check_table(const std::vector<int> &sizes)
{
    const std::vector<int> off = offsets(sizes);
    EXPECT(ragged_offsets_fault((int)sizes.size(), off.data()) == nullptr);
    check_owner(off);
    for (int shift : {6, 8, 10}) check_items(off, shift);
}

static std::string refusal(int c, const int *soff, const int *toff, const int *koff, int expect_rc)
{
    const char *what = nullptr;
    char buf[96];
    const int rc = ragged_cand_check(c, soff, toff, koff, &what, buf);
    EXPECT(rc == expect_rc);
    EXPECT((rc < 0) == (what != nullptr));
    return what ? what : "";
}

int main()
{
    // ---- the searches
    check_table({1});
    check_table({1025});
    const int kinds[8] = {0, 1, 63, 64, 65, 1023, 1024, 1025};
    for (int c = 2; c <= 6; c++) {                     // every pattern of the eight sizes, empty ones among them: 8^c tables
        int total = 1;
        for (int j = 0; j < c; j++) total *= 8;
        std::vector<int> sizes((size_t)c);
        for (int code = 0; code < total && !fails; code++) {
            for (int j = 0, rest = code; j < c; j++, rest /= 8) sizes[(size_t)j] = kinds[rest % 8];
            check_table(sizes);
        }
    }
    for (int c : {128, 256, 384}) check_table(std::vector<int>((size_t)c, 1));
    for (int at : {0, 383, 200}) {                     // all empty but the first, but the last, but one in the middle
        std::vector<int> sizes(384, 0);
        sizes[(size_t)at] = 1025;
        check_table(sizes);
    }
    {                                                  // no element at all: item j is pair j's idle one
        const std::vector<int> off(6, 0);
        for (int shift : {6, 8, 10}) check_items(off, shift);
    }

    // ---- the check
    {
        const int good[4] = {0, 0, 7, 7}, late[4] = {1, 2, 3, 4}, down[4] = {0, 5, 4, 9}, both[4] = {2, 1, 3, 4};
        EXPECT(ragged_offsets_fault(3, good) == nullptr && ragged_offsets_fault(0, good) == nullptr);
        EXPECT(!strcmp(ragged_offsets_fault(3, late), "offsets must start at 0"));
        EXPECT(!strcmp(ragged_offsets_fault(3, down), "offsets must ascend"));
        EXPECT(!strcmp(ragged_offsets_fault(3, both), "offsets must start at 0"));
        EXPECT(ragged_offsets_fault(1, down) == nullptr);          // (only the first c + 1 entries are looked at)
        // tables checked together: where any of them starts comes before how any of them ascends
        EXPECT(ragged_offsets_fault(3, {good, good}) == nullptr);
        EXPECT(!strcmp(ragged_offsets_fault(3, {down, late}), "offsets must start at 0"));
        EXPECT(!strcmp(ragged_offsets_fault(3, {good, down, good}), "offsets must ascend"));
    }

    // ---- the padded copy
    {
        const int src[4] = {0, 3, 3, 10};
        int dst[9];
        for (int c = 0; c <= 3; c++) {
            memset(dst, -1, sizeof dst);
            ragged_pad_copy(dst, src, c);
            for (int j = 0; j < 9; j++) EXPECT(dst[j] == src[j < c ? j : c]);
            EXPECT(dst[8] == src[c]);
        }
        RaggedCandTable t;
        const int s[3] = {0, 5, 9}, g[3] = {0, 4, 4}, k[3] = {0, 0, 2};
        ragged_cand_fill(t, 2, s, g, k);
        EXPECT(t.c == 2 && t.soff[1] == 5 && t.soff[kRaggedCandMaxPairs] == 9 && t.toff[kRaggedCandMaxPairs] == 4 && t.koff[kRaggedCandMaxPairs] == 2);
        EXPECT(ragged_cand_pair_of(t, 0) == 1 && ragged_cand_pair_of(t, 1) == 1);          // (pair 0 has no candidates)
        EXPECT(offsetof(RaggedCandTable, c) == 0 && offsetof(RaggedCandTable, soff) == 4 && offsetof(RaggedCandTable, toff) == 4 + 257 * 4 &&
               offsetof(RaggedCandTable, koff) == 4 + 2 * 257 * 4 && sizeof(RaggedCandTable) == 4 + 3 * 257 * 4);
    }

    // ---- the refusals genpc_icp_batch_ragged and genpc_scale_search_scores_ragged share (tests/test_icp_ragged_host.py's table)
    {
        const int n = kRaggedCandMaxPairs;
        const std::vector<int> zeros((size_t)n + 2, 0);
        const int ok[3] = {0, 5, 9}, zero[1] = {0}, late[3] = {1, 5, 9}, down[3] = {0, 9, 5};
        const int many[3] = {0, 1 << 28, (1 << 28) + 1}, cands[3] = {0, 1 << 20, (1 << 20) + 1};
        const int no_source[3] = {0, 5, 5}, no_target[3] = {0, 0, 9}, k12[3] = {0, 1, 12}, none[3] = {0, 0, 0};
        EXPECT(refusal(-1, zero, zero, zero, -1) == "negative number of pairs");
        EXPECT(refusal(n + 1, zeros.data(), zeros.data(), zeros.data(), -1) == "more than 256 pairs in one call");
        EXPECT(refusal(2, nullptr, ok, ok, -1) == "null offset table");
        EXPECT(refusal(2, ok, nullptr, ok, -1) == "null offset table");
        EXPECT(refusal(2, ok, ok, nullptr, -1) == "null offset table");
        EXPECT(refusal(2, late, ok, ok, -1) == "offsets must start at 0");
        EXPECT(refusal(2, ok, late, ok, -1) == "offsets must start at 0");
        EXPECT(refusal(2, ok, ok, late, -1) == "offsets must start at 0");
        EXPECT(refusal(2, down, ok, ok, -1) == "offsets must ascend");
        EXPECT(refusal(2, ok, down, ok, -1) == "offsets must ascend");
        EXPECT(refusal(2, ok, ok, down, -1) == "offsets must ascend");
        EXPECT(refusal(2, many, ok, ok, -1) == "more than 2^28 points on one side");
        EXPECT(refusal(2, ok, many, ok, -1) == "more than 2^28 points on one side");
        EXPECT(refusal(2, ok, ok, cands, -1) == "more than 2^20 candidates");
        EXPECT(refusal(2, no_source, ok, k12, -1) == "pair 1 has candidates and an empty source");
        EXPECT(refusal(2, ok, no_target, k12, -1) == "pair 0 has candidates and an empty target");
        // nothing to do, and work
        EXPECT(refusal(0, nullptr, nullptr, nullptr, 0) == "");
        EXPECT(refusal(2, ok, no_target, none, 0) == "");
        EXPECT(refusal(2, ok, ok, k12, 1) == "");
        EXPECT(refusal(n, zeros.data(), zeros.data(), zeros.data(), 0) == "");
        // two faults at once: the first in the order above wins
        EXPECT(refusal(-1, nullptr, nullptr, nullptr, -1) == "negative number of pairs");
        EXPECT(refusal(n + 1, nullptr, nullptr, nullptr, -1) == "more than 256 pairs in one call");
        EXPECT(refusal(2, nullptr, late, down, -1) == "null offset table");
        EXPECT(refusal(2, down, late, ok, -1) == "offsets must ascend");                 // (one table after the other: the source first)
        EXPECT(refusal(2, ok, late, down, -1) == "offsets must start at 0");
        EXPECT(refusal(2, many, ok, down, -1) == "offsets must ascend");
        EXPECT(refusal(2, many, ok, cands, -1) == "more than 2^28 points on one side");
        EXPECT(refusal(2, no_source, ok, cands, -1) == "more than 2^20 candidates");
        EXPECT(refusal(2, no_source, no_target, k12, -1) == "pair 0 has candidates and an empty target");
        const char *what = nullptr;
        EXPECT(ragged_cand_count(-1, &what) == -1 && !strcmp(what, "negative number of pairs"));
        EXPECT(ragged_cand_count(n + 1, &what) == -1 && !strcmp(what, "more than 256 pairs in one call"));
        EXPECT(ragged_cand_count(0, &what) == 0 && ragged_cand_count(1, &what) == 1 && ragged_cand_count(n, &what) == 1);
    }
    if (fails) return 1;
    printf("ragged_offsets_check: ok\n");
    return 0;
}
