// emd_ragged_plan_check.cpp -- csrc/emd_ragged_plan.h as a plain host program (tests/test_emd_ragged_plan.py builds it with the
// address and undefined-behaviour sanitizers): the launch plan of the ragged auction's bid kernel.  For every table of the
// sweep and for 1, 256 and 304 compute units: every workgroup of the grid maps to exactly one (pair, workgroup-in-pair),
// every pair with points owns at least one workgroup and an empty pair none, no pair owns more than its finest split needs
// (ceil(N_j * 64 / 256)) nor more than kEmdRaggedMaxBlocks, the grid is the sum and stays below 2^31, and every 256-point
// block of the packed arrays finds its own pair.
#include <stdio.h>
#include <vector>
#include "emd_ragged_plan.h"

using namespace genpc;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static long long tables = 0, blocks_seen = 0;

static void check(const std::vector<int> &sizes, int cus)
{
    const int c = (int)sizes.size();
    std::vector<int> off((size_t)c + 1, 0);
    for (int j = 0; j < c; j++) off[(size_t)j + 1] = off[(size_t)j] + sizes[(size_t)j];
    EmdRaggedTable t;
    const int grid = emd_ragged_plan(c, off.data(), cus, t);
    tables++;
    EXPECT(t.c == c && t.first[0] == 0 && t.first[c] == grid && t.off[c] == off[(size_t)c]);
    EXPECT((long long)grid < (1ll << 31) && grid <= c * kEmdRaggedMaxBlocks);
    for (int j = c; j <= kEmdRaggedMaxPairs; j++) EXPECT(t.first[j] == grid && t.off[j] == off[(size_t)c]);   // the tail is defined
    long long sum = 0;
    std::vector<int> owner((size_t)grid, -1);
    for (int j = 0; j < c; j++) {
        const int n = sizes[(size_t)j], g = t.first[j + 1] - t.first[j];
        EXPECT(t.off[j] == off[(size_t)j]);
        EXPECT(g >= 0);
        if (n == 0) EXPECT(g == 0);                                         // an empty pair owns nothing
        else EXPECT(g >= 1);                                                // a pair with points is served
        EXPECT((long long)g <= ((long long)n * 64 + kEmdRaggedBlock - 1) / kEmdRaggedBlock);   // the finest split: a wave per bidder
        EXPECT(g <= kEmdRaggedMaxBlocks && g == emd_ragged_blocks_of(n, off[(size_t)c], cus));
        EXPECT(emd_ragged_block_cap(n) >= (n > 0 ? 1 : 0));
        sum += g;
        for (int w = t.first[j]; w < t.first[j + 1]; w++) {
            EXPECT(owner[(size_t)w] == -1);                                 // exactly one owner
            owner[(size_t)w] = j;
            const int pair = emd_ragged_pair_of_block(t, w);
            EXPECT(pair == j);
            const int bx = w - t.first[pair];
            EXPECT(bx >= 0 && bx < g);                                      // the workgroup's number inside its pair
            blocks_seen++;
        }
        for (int pos = off[(size_t)j]; pos < off[(size_t)j + 1]; pos += 256) EXPECT(emd_ragged_pair_of_point(t, pos) == j);
        if (n > 0) EXPECT(emd_ragged_pair_of_point(t, off[(size_t)j + 1] - 1) == j);
    }
    EXPECT(sum == grid);
    for (int w = 0; w < grid; w++) EXPECT(owner[(size_t)w] >= 0);           // no workgroup without a pair
}

int main()
{
    const int cus[] = {1, 256, 304};
    for (int cu : cus) {
        check({256}, cu);                                                   // c = 1
        check({16384}, cu);
        check({1 << 20}, cu);
        check({0, 256}, cu);
        check({256, 0}, cu);
        check({0, 0, 512, 0, 0}, cu);
        check({256, 1024, 0, 768, 2304, 512, 1280}, cu);
        check({4352, 256, 256}, cu);
        check(std::vector<int>(384, 256), cu);                              // the pair-count limit
        check(std::vector<int>(384, 16384), cu);
        std::vector<int> cyc(384);
        const int three[] = {0, 256, 16384};
        for (int j = 0; j < 384; j++) cyc[(size_t)j] = three[j % 3];
        check(cyc, cu);
        std::vector<int> lone(384, 0);                                      // one pair with points among 383 without
        lone[200] = 256;
        check(lone, cu);
        check(std::vector<int>(256, 1 << 20), cu);                          // 2^28 points: the call's limit
        unsigned s = 12345u + (unsigned)cu;
        for (int rep = 0; rep < 200; rep++) {
            s = s * 1664525u + 1013904223u;
            std::vector<int> v((size_t)(1 + (s >> 8) % 40));
            for (size_t j = 0; j < v.size(); j++) {
                s = s * 1664525u + 1013904223u;
                v[j] = (int)((s >> 10) % 5 == 0 ? 0 : 256 * (1 + (s >> 12) % 70));
            }
            bool any = false;
            for (int x : v) any = any || x > 0;
            if (any) check(v, cu);
        }
    }
    // the caps by themselves
    EXPECT(emd_ragged_block_cap(256) == 64 && emd_ragged_block_cap(4096) == 1024 && emd_ragged_block_cap(1 << 28) == kEmdRaggedMaxBlocks);
    EXPECT(emd_ragged_blocks_of(0, 256, 256) == 0 && emd_ragged_blocks_of(256, 256, 0) >= 1);
    printf("tables %lld, workgroups %lld\n", tables, blocks_seen);
    if (fails) { printf("emd_ragged_plan_check: %d FAILED\n", fails); return 1; }
    printf("emd_ragged_plan_check: ok\n");
    return 0;
}
