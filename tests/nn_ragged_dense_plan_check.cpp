// Stand-alone check of genpc_amd/csrc/nn_ragged_dense_plan.h (host code only; tests/test_nn_ragged_dense_plan.py builds it with
// -fsanitize=address,undefined and runs it).  Exit status 0 = every check passed; each failure prints what it found.
// What is expected is recomputed here by brute force from the sizes: an item per 64 queries in the numbering ragged_table.h
// proves (every query of every pair is owned by exactly one item, and that item is its pair's), the sum of n_j m_j term by
// term, the two refusals from the limits as the issue states them (2^36 evaluations, 2^20 targets), typed in here.
#include "nn_ragged_dense_plan.h"

#include <stdio.h>
#include <string.h>
#include <random>
#include <vector>

using namespace genpc;

static int g_failed = 0;

static void expect(const char *what, const char *which, long long got, long long want)
{
    if (got != want) { printf("FAILED %s: %s = %lld, expected %lld\n", what, which, got, want); g_failed++; }
}

static std::vector<int> offsets(const std::vector<int> &n)
{
    std::vector<int> off(n.size() + 1, 0);          // exactly c + 1 entries: the sanitizer sees a read past them
    for (size_t j = 0; j < n.size(); j++) off[j + 1] = off[j] + n[j];
    return off;
}

// the table of a call, through ragged_table_fill as the entry points fill it; rc as it returns
static int table_of(const std::vector<int> &n, const std::vector<int> &m, RaggedTable &t)
{
    const std::vector<int> noff = offsets(n), moff = offsets(m);
    int max_targets = 0;
    const char *err = nullptr;
    return ragged_table_fill((int)n.size(), noff.data(), moff.data(), t, &max_targets, &err);
}

static void check_table(const char *what, const std::vector<int> &n, const std::vector<int> &m)
{
    RaggedTable t;
    memset(&t, 0, sizeof t);
    const int rc = table_of(n, m, t);
    long long queries = 0;
    for (int v : n) queries += v;
    expect(what, "ragged_table_fill", rc, queries > 0 ? 1 : 0);
    if (rc != 1) return;
    const NnRaggedDensePlan p = nn_ragged_dense_plan(t);
    const int c = (int)n.size();
    long long evals = 0;
    int big = 0;
    for (int j = 0; j < c; j++) {
        evals += (long long)n[j] * m[j];
        if (n[j] > 0 && m[j] > (1 << 20)) big = 1;
    }
    expect(what, "threads", p.threads, 256);
    expect(what, "queries", p.queries, 64);
    expect(what, "tile", p.tile, kNnDenseTile);
    expect(what, "share x waves", (long long)p.share * (p.threads / 64), p.tile);
    expect(what, "lds_bytes", p.lds_bytes, (long long)p.tile * 16 + (p.threads / 64) * 4);
    expect(what, "lds within a workgroup's limit", p.lds_bytes <= 64 * 1024, 1);
    expect(what, "evals", p.evals, evals);
    expect(what, "refused", p.too_large != nullptr, big || evals > (1ll << 36));
    // the items: every query is served once, by an item of its own pair, at the lane the kernel gives it
    expect(what, "items", p.items, (queries >> 6) + c);
    if (queries > (1 << 22)) return;                // (the refusal tables: their items are not walked)
    std::vector<char> seen((size_t)queries, 0);
    int idle = 0;
    for (long long item = 0; item < p.items; item++) {
        const int pair = ragged_pair_of(t, (int)item);
        if (pair < 0 || pair >= c) { expect(what, "pair in range", pair, -1); return; }
        const int q0 = t.qoff[pair], nq = t.qoff[pair + 1] - q0;
        const long long first = (item - ((q0 >> 6) + pair)) * p.queries;
        if (first < 0) { expect(what, "first query of an item", first, 0); return; }
        if (first >= nq) { idle++; continue; }
        for (int lane = 0; lane < p.queries && first + lane < nq; lane++) seen[(size_t)q0 + first + lane]++;
    }
    long long once = 0;
    for (char s : seen) once += s == 1;
    expect(what, "queries served exactly once", once, queries);
    expect(what, "idle items at most one per pair", idle <= c, 1);
}

int main()
{
    std::mt19937 rng(20261020);
    check_table("one pair", {300}, {24000});
    check_table("single points", {1, 1, 1}, {1, 1, 1});
    check_table("empty pairs in the middle and at the end", {65, 0, 64, 0}, {7, 0, 1025, 3});
    check_table("no queries at all", {0, 0}, {5, 0});
    check_table("queries without work beside it", {0, 63}, {100, 1});
    for (int c : {1, 2, 36, 384})
        for (int round = 0; round < 6; round++) {
            std::vector<int> n(c), m(c);
            for (int j = 0; j < c; j++) {
                const int kind = (int)(rng() % 8);
                n[j] = kind == 0 ? 0 : (kind == 1 ? 1 : (int)(rng() % 700));
                m[j] = kind == 2 ? 1 : 1 + (int)(rng() % 5000);
                if (kind == 3) { n[j] = 0; m[j] = 0; }
            }
            char what[64];
            snprintf(what, sizeof what, "random table, c = %d, round %d", c, round);
            check_table(what, n, m);
        }

    // the evaluation limit: 2^36 = 2^18 x 2^18 -- one below, at, one above; and the issue's case, n = m = 2^18 + 1
    const int h = 1 << 18;
    check_table("2^36 - 2^18 evaluations", {h - 1}, {h});
    check_table("2^36 evaluations", {h}, {h});
    check_table("2^36 + 2^18 evaluations", {h + 1}, {h});
    check_table("n = m = 2^18 + 1", {h + 1}, {h + 1});
    check_table("2^36 + 1 evaluations over two pairs", {h, 1}, {h, 1});
    // the target limit: 2^20 -- one below, at, one above; a pair WITHOUT queries may be as large as it likes
    const int k = 1 << 20;
    check_table("2^20 - 1 targets", {3}, {k - 1});
    check_table("2^20 targets", {3}, {k});
    check_table("2^20 + 1 targets", {3}, {k + 1});
    check_table("2^20 + 1 targets in a pair without queries", {0, 5}, {k + 1, 9});
    {
        RaggedTable t;
        memset(&t, 0, sizeof t);
        table_of({3}, {k + 1}, t);
        const NnRaggedDensePlan p = nn_ragged_dense_plan(t);
        expect("the target refusal", "names 2^20", p.too_large && strstr(p.too_large, "2^20") != nullptr, 1);
        table_of({h + 1}, {h + 1}, t);
        const NnRaggedDensePlan q = nn_ragged_dense_plan(t);
        expect("the evaluation refusal", "names 2^36", q.too_large && strstr(q.too_large, "2^36") != nullptr, 1);
    }
    if (g_failed) { printf("nn_ragged_dense_plan_check: %d FAILED\n", g_failed); return 1; }
    printf("nn_ragged_dense_plan_check: ok\n");
    return 0;
}
