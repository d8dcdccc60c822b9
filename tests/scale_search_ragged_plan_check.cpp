// Stand-alone check of genpc_amd/csrc/scale_search_ragged_plan.h (host code only; tests/test_scale_search_ragged_plan.py builds it
// with -fsanitize=address,undefined and runs it).  Exit status 0 = every check passed; each failure prints what it found.
// The LDS arithmetic is restated here by hand from the layout in the header's comment (fixed part, 16 bytes a point, a table of
// cells + 1 ints rounded to 16 bytes) for every ns up to the boundary and past it; the split of a table is counted pair by pair.
#include "scale_search_ragged_plan.h"

#include <stdio.h>
#include <vector>

using namespace genpc;

static int g_failed = 0;

static void expect(const char *what, const char *which, long long got, long long want)
{
    if (got != want) { printf("FAILED %s: %s = %lld, expected %lld\n", what, which, got, want); g_failed++; }
}

static void check(const char *what, const std::vector<int> &nss, int fused, int loop, int lds)
{
    std::vector<int> soff(nss.size() + 1, 0);          // exactly c + 1 entries: the sanitizer sees a read past them
    for (size_t j = 0; j < nss.size(); j++) soff[j + 1] = soff[j] + nss[j];
    const ScaleSearchRaggedPlan p = scale_search_ragged_plan((int)nss.size(), soff.data());
    expect(what, "fused_pairs", p.fused_pairs, fused);
    expect(what, "loop_pairs", p.loop_pairs, loop);
    expect(what, "lds_bytes", p.lds_bytes, lds);
}

int main()
{
    // the fixed part: per wave 6 floats of the box, 2 ints of the scan, 2 doubles of the score; a multiple of 16
    expect("layout", "kSsFixed", (long long)kSsFixed, 4 * (6 * 4 + 2 * 4 + 2 * 8));
    expect("layout", "kSsFixed % 16", (long long)(kSsFixed % 16), 0);
    // every ns up to the boundary and past it
    int last = 0, prev_cells = 0;
    const long long room = (long long)kSsLdsBudget - (long long)kSsLdsReserve;
    for (int ns = -2; ns <= 12000; ns++) {
        const ScaleSearchPlan p = scale_search_plan(ns);
        if (ns <= 0) {
            if (p.one_workgroup || p.cells || p.lds_bytes) { printf("FAILED: ns %d has a plan\n", ns); g_failed++; }
            continue;
        }
        if (!p.one_workgroup) {
            if (p.cells || p.lds_bytes) { printf("FAILED: ns %d: the single call with cells or LDS\n", ns); g_failed++; }
            // not even the smallest budget the halving reaches fits
            int least_cells = ragged_cells_max(ns);
            while (least_cells >= 2 * kSsCellsMin) least_cells >>= 1;
            const long long least = (long long)kSsFixed + 16LL * ns + ((long long)least_cells + 1 + 3) / 4 * 16;
            if (least <= room) { printf("FAILED: ns %d would fit with %d cells\n", ns, least_cells); g_failed++; }
            continue;
        }
        if (last != ns - 1) { printf("FAILED: the plan is not monotone: ns %d fused after ns %d was not\n", ns, ns - 1); g_failed++; }
        last = ns;
        const long long want = (long long)kSsFixed + 16LL * ns + ((long long)p.cells + 1 + 3) / 4 * 16;
        if (p.lds_bytes != want) { printf("FAILED: ns %d: lds %d, by hand %lld\n", ns, p.lds_bytes, want); g_failed++; }
        if (p.lds_bytes > room) { printf("FAILED: ns %d: %d bytes do not fit\n", ns, p.lds_bytes); g_failed++; }
        if (p.lds_bytes % 16) { printf("FAILED: ns %d: lds %d is no multiple of 16\n", ns, p.lds_bytes); g_failed++; }
        // the cell budget: the ragged build's for this count, halved (never below kSsCellsMin by halving) only when it must be
        int c = ragged_cells_max(ns);
        bool halved = false;
        while (c != p.cells && c >= 2 * kSsCellsMin) { c >>= 1; halved = true; }
        if (c != p.cells) { printf("FAILED: ns %d: %d cells is no halving of %d\n", ns, p.cells, ragged_cells_max(ns)); g_failed++; }
        if (halved && (long long)kSsFixed + 16LL * ns + ((long long)p.cells * 2 + 1 + 3) / 4 * 16 <= room) {
            printf("FAILED: ns %d: twice %d cells would fit\n", ns, p.cells); g_failed++;
        }
        if (p.cells < 1 || (p.cells < kSsCellsMin && p.cells != ragged_cells_max(ns))) { printf("FAILED: ns %d: %d cells\n", ns, p.cells); g_failed++; }
        const int t = scale_search_cells_target(ns, p.cells);
        if (t < 1 || t > p.cells || t > ragged_cells_target(ns)) { printf("FAILED: ns %d: cell target %d of %d\n", ns, t, p.cells); g_failed++; }
        prev_cells = p.cells;
    }
    (void)prev_cells;
    if (last < 2500 || last >= 12000) { printf("FAILED: the boundary %d is not where the pipeline's clouds need it\n", last); g_failed++; }
    const int first_loop = last + 1;
    expect("boundary", "2^24 - 1 is the single call's", scale_search_plan((1 << 24) - 1).one_workgroup, 0);
    expect("boundary", "2^24 is the single call's", scale_search_plan(1 << 24).one_workgroup, 0);
    expect("boundary", "2^28 is the single call's", scale_search_plan(1 << 28).one_workgroup, 0);

    // the split of a table
    check("no pair", {}, 0, 0, 0);
    {
        const ScaleSearchRaggedPlan p = scale_search_ragged_plan(0, nullptr);
        expect("no pair, null table", "sum", p.fused_pairs + p.loop_pairs + p.lds_bytes, 0);
    }
    check("ns 1", {1}, 1, 0, scale_search_plan(1).lds_bytes);
    check("the last fused ns", {last}, 1, 0, scale_search_plan(last).lds_bytes);
    check("the first ns of the single call", {first_loop}, 0, 1, 0);
    check("mixed", {0, 700, first_loop, last, 0, 1, first_loop + 5000}, 3, 2, scale_search_plan(last).lds_bytes);
    check("mixed, reversed", {first_loop + 5000, 1, 0, last, first_loop, 700, 0}, 3, 2, scale_search_plan(last).lds_bytes);
    check("all of the single call", {first_loop, 20000}, 0, 2, 0);
    check("all empty", {0, 0, 0}, 0, 0, 0);
    {
        std::vector<int> nss(kSsRaggedMaxPairs, 1);
        nss[kSsRaggedMaxPairs - 1] = first_loop;
        nss[7] = 2500;
        check("256 pairs", nss, kSsRaggedMaxPairs - 1, 1, scale_search_plan(2500).lds_bytes);
    }
    // three offset tables of kSsRaggedMaxPairs + 1 ints and what else the launch takes fit the 4 KiB of kernel arguments
    if ((size_t)3 * (kSsRaggedMaxPairs + 1) * sizeof(int) + 128 > 4096) { printf("FAILED: the tables do not fit the kernel arguments\n"); g_failed++; }

    if (g_failed) {
        printf("scale_search_ragged_plan_check: %d check(s) failed\n", g_failed);
        return 1;
    }
    printf("scale_search_ragged_plan_check: ok (one workgroup up to ns %d)\n", last);
    return 0;
}
