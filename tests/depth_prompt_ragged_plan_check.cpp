// Stand-alone check of genpc_amd/csrc/depth_prompt_ragged_plan.h (host code only; tests/test_depth_prompt_ragged_plan.py builds
// it with -fsanitize=address,undefined and runs it).  Exit status 0 = every check passed; each failure prints what it found.
// The item numbering is checked by brute force against the table: every scan's chunks get items of their own, in ascending
// order, and the search finds the scan of every item.
#include "depth_prompt_ragged_plan.h"

#include <stdio.h>
#include <string.h>
#include <vector>

using namespace genpc;

static int g_failed = 0;

static void expect(const char *what, const char *which, long long got, long long want)
{
    if (got != want) { printf("FAILED %s: %s = %lld, expected %lld\n", what, which, got, want); g_failed++; }
}

static void refused(const char *what, int c, const int *off, int res, int ps, int rate, const char *msg)
{
    const char *e = depth_prompt_ragged_fault(c, off, res, ps, rate);
    if (!e || !strstr(e, msg)) { printf("FAILED %s: got '%s', expected '%s'\n", what, e ? e : "(taken)", msg); g_failed++; }
}

static void numbering(const char *what, const std::vector<int> &ns)
{
    const int c = (int)ns.size();
    std::vector<int> off(c + 1, 0);                     // exactly c + 1 entries: the sanitizer sees a read past them
    for (int j = 0; j < c; j++) off[j + 1] = off[j] + ns[j];
    if (depth_prompt_ragged_fault(c, off.data(), 64, 1, 3)) { printf("FAILED %s: refused\n", what); g_failed++; return; }
    const DepthPromptRaggedPlan p = depth_prompt_ragged_plan(c, off.data(), 64);
    DepthPromptRaggedTable t;
    t.c = c;
    ragged_pad_copy(t.off, off.data(), c);
    expect(what, "items", p.items, (off[c] >> 10) + c);
    expect(what, "launches", p.launches, 4);
    expect(what, "memsets", p.memsets, 1);
    std::vector<int> owner(p.items, -1);
    long long covered = 0;
    int refusedn = 0, first = -1;
    for (int j = 0; j < c; j++) {
        if (ns[j] == 0) { refusedn++; if (first < 0) first = j; }
        const int f = depth_prompt_first_item(t.off, j), k = depth_prompt_chunks(ns[j]);
        if (j + 1 < c && f + k > depth_prompt_first_item(t.off, j + 1)) { printf("FAILED %s: scan %d runs into scan %d\n", what, j, j + 1); g_failed++; }
        if (f + k > p.items) { printf("FAILED %s: scan %d needs item %d of %d\n", what, j, f + k - 1, p.items); g_failed++; continue; }
        for (int q = 0; q < k; q++) {
            if (owner[f + q] != -1) { printf("FAILED %s: item %d taken twice\n", what, f + q); g_failed++; }
            owner[f + q] = j;
            const int lo = q << kDpChunkShift, hi = lo + kDpChunk < ns[j] ? lo + kDpChunk : ns[j];
            covered += hi - lo;
        }
    }
    expect(what, "points covered", covered, off[c]);
    expect(what, "refused", p.refused, refusedn);
    expect(what, "first_refused", p.first_refused, first);
    for (int item = 0; item < p.items; item++) {
        const int j = depth_prompt_scan_of(t, item);
        if (j < 0 || j >= c) { printf("FAILED %s: item %d -> scan %d\n", what, item, j); g_failed++; continue; }
        if (owner[item] >= 0 && owner[item] != j) { printf("FAILED %s: item %d belongs to scan %d, found %d\n", what, item, owner[item], j); g_failed++; }
        // a spare item finds a scan whose chunks end before it: nothing to do
        const int base = (item - depth_prompt_first_item(t.off, j)) << kDpChunkShift;
        if (owner[item] < 0 && base < ns[j]) { printf("FAILED %s: spare item %d has work in scan %d\n", what, item, j); g_failed++; }
    }
    expect(what, "fill_ints", p.fill_ints, 12LL * c + 2LL * c * 64 * 64);
    expect(what, "ws_bytes", p.ws_bytes, p.fill_ints * 4 + 16LL * p.items + 32LL * c);
}

int main()
{
    expect("constants", "kDpChunk", kDpChunk, 1024);
    expect("constants", "kDpLaunches", kDpLaunches, 4);
    expect("constants", "kDpMemsets", kDpMemsets, 1);
    expect("constants", "kDpKeysPerScan", kDpKeysPerScan, 12);
    if (sizeof(DepthPromptRaggedTable) + 256 > 4096) { printf("FAILED: the table does not fit the kernel arguments\n"); g_failed++; }

    // the limits
    const int ok[3] = {0, 5, 9};
    if (depth_prompt_ragged_fault(2, ok, 64, 2, 3)) { printf("FAILED: a plain call is refused\n"); g_failed++; }
    if (depth_prompt_ragged_fault(0, nullptr, 64, 1, 3)) { printf("FAILED: no scan is refused\n"); g_failed++; }
    if (depth_prompt_ragged_fault(2, ok, kDpMaxRes, 1, 3)) { printf("FAILED: res 4096 with two scans is refused\n"); g_failed++; }
    if (depth_prompt_ragged_fault(2, ok, 64, 4, 8)) { printf("FAILED: a stamp of 32 is refused\n"); g_failed++; }
    refused("c < 0", -1, ok, 64, 1, 3, "negative number of scans");
    {
        std::vector<int> z(kDpMaxScans + 2, 0);
        refused("c > max", kDpMaxScans + 1, z.data(), 64, 1, 3, "more than 256 scans");
        if (depth_prompt_ragged_fault(kDpMaxScans, z.data(), 64, 1, 3)) { printf("FAILED: 256 scans are refused\n"); g_failed++; }
        refused("owner planes", kDpMaxScans, z.data(), 4096, 1, 3, "owner planes");
    }
    refused("res 0", 2, ok, 0, 1, 3, "res outside");
    refused("res 4097", 2, ok, 4097, 1, 3, "res outside");
    refused("point_size 0", 2, ok, 64, 0, 3, "must be positive");
    refused("rate 0", 2, ok, 64, 1, 0, "must be positive");
    refused("stamp 33", 2, ok, 64, 11, 3, "above 32");
    refused("stamp overflow", 2, ok, 64, 1 << 20, 1 << 20, "above 32");
    refused("null table", 2, nullptr, 64, 1, 3, "null offset table");
    { const int b[3] = {1, 5, 9}; refused("start", 2, b, 64, 1, 3, "offsets must start at 0"); }
    { const int b[3] = {0, 9, 5}; refused("descends", 2, b, 64, 1, 3, "offsets must ascend"); }
    { const int b[3] = {0, 1 << 28, (1 << 28) + 1}; refused("points", 2, b, 64, 1, 3, "more than 2^28 points"); }

    // the numbering, the launch count and the refusal of empty scans
    numbering("the GPU test's batch", {1, 2, 257, 300, 5000});
    numbering("reversed", {5000, 300, 257, 2, 1});
    numbering("an empty scan in the middle", {300, 0, 5000});
    numbering("all empty", {0, 0, 0});
    numbering("chunk boundaries", {1023, 1024, 1025, 2048, 1, 4097, 0, 1024});
    numbering("one scan", {12000});
    {
        std::vector<int> ns(kDpMaxScans, 3);
        ns[17] = 0; ns[200] = 70000;
        numbering("256 scans", ns);
    }
    {
        const DepthPromptRaggedPlan p = depth_prompt_ragged_plan(0, nullptr, 64);
        expect("no scan", "launches + items + memsets", p.launches + p.items + p.memsets, 0);
    }
    if (g_failed) {
        printf("depth_prompt_ragged_plan_check: %d check(s) failed\n", g_failed);
        return 1;
    }
    printf("depth_prompt_ragged_plan_check: ok\n");
    return 0;
}
