// ragged_table_check.cpp -- csrc/ragged_table.h as a plain host program (tests/test_nn_ragged_host.py builds it with the
// address and undefined-behaviour sanitizers): the offset checks, the copy into the table, and the two placements that replace
// prefix sums on the device -- a pair's cell table inside `start`, a pair's workgroups inside the launch.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "ragged_table.h"

using namespace genpc;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static int fill(const std::vector<int> &n, const std::vector<int> &m, RaggedTable &t, int *mx, const char **err)
{
    return ragged_table_fill((int)n.size() - 1, n.data(), m.data(), t, mx, err);
}

// every placement the kernels derive from a valid table
static void placements(const RaggedTable &t)
{
    const int c = t.c;
    const long long items = ragged_items(t.qoff[c], c), slen = ragged_start_len(t.toff[c], c);
    std::vector<int> owner((size_t)items, -1);
    long long queries = 0;
    for (int j = 0; j < c; j++) {
        const int n = t.qoff[j + 1] - t.qoff[j], m = t.toff[j + 1] - t.toff[j];
        // cell table: [toff[j] + 65 j, toff[j + 1] + 65 (j + 1)) holds cells_max + 1 entries
        const long long s0 = (long long)t.toff[j] + (long long)kRaggedStartPad * j, s1 = (long long)t.toff[j + 1] + (long long)kRaggedStartPad * (j + 1);
        EXPECT(ragged_cells_max(m) + 1 <= s1 - s0 && s1 <= slen && s0 >= 0);
        EXPECT(ragged_cells_max(m) <= kRaggedCellsCap && ragged_cells_max(m) >= 1);
        EXPECT(ragged_cells_target(m) >= 1 && ragged_cells_target(m) <= ragged_cells_max(m));
        // workgroups: first (qoff[j] >> 6) + j, ceil(n / 64) of them, below the next pair's first
        const long long first = (t.qoff[j] >> 6) + j, need = (n + kRaggedLanes - 1) / kRaggedLanes;
        const long long next = j + 1 < c ? (t.qoff[j + 1] >> 6) + j + 1 : items;
        EXPECT(first + need <= next && next <= items);
        for (long long w = first; w < next; w++) {
            EXPECT(owner[(size_t)w] == -1);
            owner[(size_t)w] = j;
            EXPECT(ragged_pair_of(t, (int)w) == j);
            const long long lanes = n - (w - first) * kRaggedLanes;
            queries += lanes < 0 ? 0 : (lanes > kRaggedLanes ? kRaggedLanes : lanes);
        }
    }
    for (long long w = 0; w < items; w++) EXPECT(owner[(size_t)w] >= 0);
    EXPECT(queries == t.qoff[c]);
}

int main()
{
    RaggedTable t;
    int mx = 0;
    const char *err = nullptr;
    // refusals
    EXPECT(ragged_table_fill(-1, nullptr, nullptr, t, &mx, &err) == -1 && err);
    EXPECT(ragged_table_fill(0, nullptr, nullptr, t, &mx, &err) == 0 && !err);
    EXPECT(ragged_table_fill(2, nullptr, nullptr, t, &mx, &err) == -1 && err);
    EXPECT(fill({1, 2, 3}, {0, 1, 2}, t, &mx, &err) == -1 && err);
    EXPECT(fill({0, 2, 3}, {1, 1, 2}, t, &mx, &err) == -1 && err);
    EXPECT(fill({0, 3, 2}, {0, 1, 2}, t, &mx, &err) == -1 && err);
    EXPECT(fill({0, 2, 3}, {0, 2, 1}, t, &mx, &err) == -1 && err);
    EXPECT(fill({0, 2, 3}, {0, 2, 2}, t, &mx, &err) == -1 && err);                   // queries, no targets
    EXPECT(fill({0, 2, 2}, {0, 2, 2}, t, &mx, &err) == 1 && !err && mx == 2);        // neither: legal
    EXPECT(fill({0, 0, 0}, {0, 5, 9}, t, &mx, &err) == 0 && !err);                   // no queries at all
    EXPECT(fill({0, kRaggedMaxPoints + 1}, {0, 1}, t, &mx, &err) == -1 && err);
    EXPECT(fill({0, 1}, {0, kRaggedMaxPoints + 1}, t, &mx, &err) == -1 && err);
    {
        std::vector<int> z((size_t)kRaggedMaxPairs + 2, 0);
        EXPECT(ragged_table_fill(kRaggedMaxPairs + 1, z.data(), z.data(), t, &mx, &err) == -1 && err);
    }
    // the copy, and what follows from it
    EXPECT(fill({0, 63, 63, 64, 129, 129, 1154}, {0, 1, 1, 3001, 3008, 3008, 30000}, t, &mx, &err) == 1);
    EXPECT(t.c == 6 && t.qoff[6] == 1154 && t.toff[3] == 3001 && t.qoff[kRaggedMaxPairs] == 1154 && mx == 26992);
    placements(t);
    // the full table: the largest c at the largest totals, then pseudo-random sizes with empty clouds among them
    {
        std::vector<int> n((size_t)kRaggedMaxPairs + 1), m((size_t)kRaggedMaxPairs + 1);
        for (int j = 0; j <= kRaggedMaxPairs; j++) {
            n[(size_t)j] = (int)((long long)kRaggedMaxPoints * j / kRaggedMaxPairs);
            m[(size_t)j] = (int)((long long)kRaggedMaxPoints * j / kRaggedMaxPairs);
        }
        EXPECT(fill(n, m, t, &mx, &err) == 1);
        placements(t);
        unsigned s = 12345u;
        for (int rep = 0; rep < 50; rep++) {
            const int c = 1 + (int)((s = s * 1664525u + 1013904223u) >> 8) % kRaggedMaxPairs;
            n.assign((size_t)c + 1, 0);
            m.assign((size_t)c + 1, 0);
            for (int j = 0; j < c; j++) {
                const int a = (int)((s = s * 1664525u + 1013904223u) >> 8) % 700, b = (int)((s = s * 1664525u + 1013904223u) >> 8) % 40000;
                const int nn = a % 7 == 0 ? 0 : a;
                n[(size_t)j + 1] = n[(size_t)j] + nn;
                m[(size_t)j + 1] = m[(size_t)j] + (nn == 0 && b % 2 ? 0 : b + 1);
            }
            const int rc = fill(n, m, t, &mx, &err);
            EXPECT(rc == (n[(size_t)c] ? 1 : 0));
            if (rc == 1) placements(t);
        }
    }
    if (fails) return 1;
    printf("ragged_table_check: ok\n");
    return 0;
}
