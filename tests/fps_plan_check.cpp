// fps_plan_check -- csrc/fps_plan.h by itself (plain C++, built with the address and undefined-behaviour sanitizers by
// tests/test_fps_plan.py): the three ranges and their boundaries, force_large, the refusals, every workspace count monotone
// in n, and every packed field of the large sampler holding its maximum at the limit; then the decisions of a call -- the register
// classes, a cloud's co-residency shape on small, partitioned and full devices, the grouping of clouds into launches, the
// verification's segments, the workspace counts and a deferred check's buffer -- by their properties and against recorded results.
#include "fps_plan.h"

#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>

using namespace genpc;

static int g_fail = 0;
#define EXPECT(cond)                                                            \
    do {                                                                        \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); g_fail++; } \
    } while (0)

// ---- the decisions of a call: register classes, co-residency shapes, launches, verification segments, workspace

// the devices the plan is exercised on: small, partitioned and full parts; per-class occupancies uniform, and the pattern measured
// on gfx950 (four and more workgroups per CU for the small classes, three for class 16, two for class 24)
static const int kCus[6] = {1, 8, 32, 64, 256, 304};
static const int kOcc[5][kFpsClasses] = {{1, 1, 1, 1, 1, 1}, {2, 2, 2, 2, 2, 2}, {4, 4, 4, 4, 4, 4}, {8, 8, 8, 8, 8, 8}, {4, 4, 4, 4, 3, 2}};
static FpsDevice device(int cus, int pattern)
{
    FpsDevice d;
    d.cus = cus;
    for (int i = 0; i < kFpsClasses; i++) d.blocks_per_cu[i] = kOcc[pattern][i];
    return d;
}
static int points_per_thread(int n, int W) { return ((n + W - 1) / W + kFThreads - 1) / kFThreads; }
static int asked_workgroups(int n)
{
    const int W = (n + kFPointsPerWg - 1) / kFPointsPerWg;
    return W > kFMaxW ? kFMaxW : W;
}
// W workgroups hold the cloud in registers and the device holds them
static bool feasible(int n, int W, const FpsDevice &d)
{
    const int R = points_per_thread(n, W);
    return R <= kFMaxR && W <= fps_budget(d, R);
}

static void check_classes()
{
    // every R takes the smallest class that holds it; the boundaries are the instantiations' points per thread
    for (int R = 1; R <= kFMaxR; R++) {
        const int cls = fps_class(R);
        EXPECT(cls >= 0 && cls < kFpsClasses && kFpsClassPoints[cls] >= R);
        EXPECT(cls == 0 || kFpsClassPoints[cls - 1] < R);
    }
    for (int i = 1; i < kFpsClasses; i++) EXPECT(kFpsClassPoints[i] > kFpsClassPoints[i - 1]);
    EXPECT(fps_class(0) == 0 && fps_class(kFMaxR + 1) == kFpsClasses - 1);
    EXPECT(fps_class(2) == 0 && fps_class(3) == 1 && fps_class(8) == 2 && fps_class(9) == 3 && fps_class(13) == 4 && fps_class(17) == 5);
    EXPECT(kFThreads == 192 && kFMaxR == 24 && kFMaxW == 64 && kFMaxJobs == 8 && kFPointsPerWg == 192 && kFVMaxSeg == 16);
    EXPECT((long long)kFMaxW * kFMaxR * kFThreads >= kFpsMultiMaxN);
}

static void check_multi_shape()
{
    for (int cus : kCus)
        for (int pattern = 0; pattern < 5; pattern++) {
            const FpsDevice d = device(cus, pattern);
            for (int n = 1; n <= kFpsMultiMaxN && !g_fail; n++) {
                const FpsShape s = fps_multi_shape(n, d);
                const int W0 = asked_workgroups(n);
                if (s.ok) {
                    EXPECT(1 <= s.W && s.W <= kFMaxW && 1 <= s.R && s.R <= kFMaxR);
                    EXPECT(s.W <= cus * d.blocks_per_cu[fps_class(s.R)]);
                    EXPECT((long long)s.W * s.R * kFThreads >= n);
                    EXPECT(s.R == points_per_thread(n, s.W) && s.W <= W0);
                    // ... and no number of workgroups between that and what the size asks for would do
                    for (int W = s.W + 1; W <= W0; W++) EXPECT(!feasible(n, W, d));
                } else {
                    // refused only when no W the device holds keeps the points within kFMaxR per thread (the loop's path is
                    // every W from what the size asks for downwards; a W it skips exceeds the budget of a larger W, and with fewer
                    // workgroups R and the class only grow -- of a larger class a CU holds no more, on every device above)
                    for (int W = 1; W <= W0; W++) EXPECT(!feasible(n, W, d));
                }
                // a device of at least kFMaxW CUs holds every cloud's workgroups as asked (an occupancy is at least 1)
                if (cus >= kFMaxW) EXPECT(s.ok && s.W == W0);
            }
        }
    // recorded: (n, cus, occupancy pattern) -> (ok, W, R) where the budget binds
    static const int rec[][6] = {
        {193, 1, 0, 1, 1, 2},      {1000, 1, 0, 1, 1, 6},     {4608, 1, 0, 1, 1, 24},    {4609, 1, 0, 0, 0, 0},     {262144, 1, 0, 0, 0, 0},
        {1000, 1, 2, 1, 4, 2},     {4609, 1, 2, 1, 4, 7},     {9217, 1, 2, 1, 4, 13},    {50000, 1, 2, 0, 0, 0},    {4609, 1, 4, 1, 4, 7},
        {9217, 1, 4, 0, 0, 0},     {1000, 2, 0, 1, 2, 3},     {4609, 2, 0, 1, 2, 13},    {9217, 2, 0, 0, 0, 0},     {4608, 2, 2, 1, 8, 3},
        {9217, 2, 2, 1, 8, 7},     {24577, 2, 2, 1, 8, 17},   {50000, 2, 2, 0, 0, 0},    {4609, 2, 4, 1, 8, 4},     {24577, 2, 4, 0, 0, 0},
        {4609, 4, 0, 1, 4, 7},     {24577, 4, 0, 0, 0, 0},    {9217, 4, 2, 1, 16, 4},    {50000, 4, 2, 1, 16, 17},  {100000, 4, 2, 0, 0, 0},
        {24577, 4, 4, 1, 16, 9},   {50000, 4, 4, 0, 0, 0},    {4609, 8, 0, 1, 8, 4},     {24577, 8, 0, 1, 8, 17},   {262144, 8, 0, 0, 0, 0},
        {24577, 8, 2, 1, 32, 5},   {24577, 8, 4, 1, 32, 5},   {262144, 8, 4, 0, 0, 0},   {9217, 16, 0, 1, 16, 4},   {50000, 16, 0, 1, 16, 17},
        {100000, 16, 0, 0, 0, 0},  {165546, 16, 4, 0, 0, 0},
    };
    for (const auto &r : rec) {
        const FpsShape s = fps_multi_shape(r[0], device(r[1], r[2]));
        EXPECT(s.ok == (r[3] != 0));
        if (s.ok) EXPECT(s.W == r[4] && s.R == r[5]);
    }
}

static unsigned g_lcg = 12345u;
static int rnd(int below) { g_lcg = g_lcg * 1664525u + 1013904223u; return (int)((g_lcg >> 8) % (unsigned)below); }

// the launches of the clouds n[0 .. cb) on d; false: a cloud is refused
static bool check_launches_of(int cb, const int *n, const FpsDevice &d, int expect_launches, const int *expect_counts)
{
    FpsShape shape[32];
    FpsLaunch la[32];
    int slot0[32], sampler[32], k[32];
    for (int q = 0; q < cb; q++) {
        shape[q] = fps_multi_shape(n[q], d);
        if (!shape[q].ok) return false;
        sampler[q] = kFpsMulti;
        k[q] = 1;
    }
    const int nl = fps_multi_launches(cb, shape, d, la, slot0);
    EXPECT(nl >= 1 && nl <= cb);
    int next = 0, slot = 0;
    for (int i = 0; i < nl; i++) {
        const FpsLaunch &l = la[i];
        EXPECT(l.first == next && l.count >= 1 && l.count <= kFMaxJobs && l.first + l.count <= cb);      // every cloud once, in call order
        int wmax = 0, rmax = 1;
        for (int q = l.first; q < l.first + l.count; q++) {
            wmax = shape[q].W > wmax ? shape[q].W : wmax;
            rmax = shape[q].R > rmax ? shape[q].R : rmax;
            EXPECT(slot0[q] == slot);
            slot += 2 * shape[q].W;
        }
        EXPECT(l.wmax == wmax && l.rmax == rmax);
        if (l.count > 1) EXPECT((long long)l.wmax * l.count <= fps_budget(d, l.rmax));
        const int per_cu = d.blocks_per_cu[fps_class(l.rmax)];
        EXPECT(l.units == l.wmax * l.count * ((4 + per_cu - 1) / per_cu));
        next = l.first + l.count;
        // a launch ends when it is full, when no cloud is left, or when the next one would not be resident with it
        if (l.count < kFMaxJobs && next < cb) {
            const int wm = shape[next].W > wmax ? shape[next].W : wmax, rm = shape[next].R > rmax ? shape[next].R : rmax;
            EXPECT((long long)wm * (l.count + 1) > fps_budget(d, rm));
        }
        if (expect_counts) EXPECT(i < expect_launches && l.count == expect_counts[i]);
    }
    EXPECT(next == cb);
    EXPECT((size_t)slot == fps_workspace(cb, n, k, sampler, cb, shape).slots);      // the last slot0 + 2 W: what the call reserves
    if (expect_counts) EXPECT(nl == expect_launches);
    return true;
}

static void check_multi_launches()
{
    int n[32];
    for (int cus : kCus)
        for (int pattern = 0; pattern < 5; pattern++) {
            const FpsDevice d = device(cus, pattern);
            for (int trial = 0; trial < 200; trial++) {
                const int cb = 1 + rnd(20), top = rnd(2) ? 4000 : kFpsMultiMaxN;
                for (int q = 0; q < cb; q++) n[q] = 1 + rnd(top);
                (void)check_launches_of(cb, n, d, 0, nullptr);
            }
        }
    // 9 and 17 equal small clouds: 8 + 1 and 8 + 8 + 1
    for (int q = 0; q < 17; q++) n[q] = 1000;
    const int nine[2] = {8, 1}, seventeen[3] = {8, 8, 1};
    EXPECT(check_launches_of(9, n, device(256, 4), 2, nine));
    EXPECT(check_launches_of(17, n, device(256, 4), 3, seventeen));
    // the budget cuts a launch short: 64 workgroups each, a device that holds 128 of the class
    for (int q = 0; q < 5; q++) n[q] = 100000;
    const int pairs[3] = {2, 2, 1};
    EXPECT(check_launches_of(5, n, device(64, 1), 3, pairs));
}

static void check_verify_segments()
{
    for (int cus : kCus)
        for (int nj = 1; nj <= kFMaxJobs; nj++)
            for (int nmax = 1; nmax <= kFpsLargeMaxN; nmax += nmax < 3000 ? 1 : 4099) {
                const int nseg = fps_verify_segments(nmax, nj, cus, false);
                EXPECT(nseg >= 1 && nseg <= kFVMaxSeg);
                EXPECT(fps_verify_segments(nmax, nj, cus, true) == 1);
                // about four blocks per CU: never more than that, unless one segment alone is more
                const long long blocks = (long long)((nmax + kFVBlock - 1) / kFVBlock) * nj;
                EXPECT(nseg == 1 || blocks * nseg <= 4ll * cus);
            }
    // recorded: (nmax, nj, cus, single) -> segments
    static const int rec[][5] = {{24000, 1, 256, 0, 5}, {24000, 2, 256, 0, 2}, {8192, 1, 256, 0, 16}, {8192, 8, 256, 0, 2}, {100, 1, 256, 0, 16},
                                 {262144, 1, 256, 0, 1}, {165546, 4, 256, 0, 1}, {16384, 1, 32, 0, 1}, {20000, 3, 64, 0, 1}, {1, 1, 1, 0, 4},
                                 {300000, 1, 256, 1, 1}, {1000, 1, 256, 1, 1}, {3000, 8, 304, 0, 6}};
    for (const auto &r : rec) EXPECT(fps_verify_segments(r[0], r[1], r[2], r[3] != 0) == r[4]);
}

// the workspace of a call of the clouds n[0 .. c), k[0 .. c) on a full device; multi_only: the genpc_fps_tune(256) hook
static FpsWorkspace workspace_of(int c, const int *n, const int *k, int force_large, bool multi_only)
{
    const FpsDevice d = device(256, 4);
    int sampler[8], cb = 0;
    FpsShape shape[8];
    for (int j = 0; j < c; j++) {
        sampler[j] = fps_plan(n[j], force_large).sampler;
        if (sampler[j] == kFpsGrid && multi_only) sampler[j] = kFpsMulti;
        if (sampler[j] == kFpsMulti) shape[cb++] = fps_multi_shape(n[j], d);
    }
    return fps_workspace(c, n, k, sampler, cb, shape);
}
static bool no_less(const FpsWorkspace &a, const FpsWorkspace &b)
{
    return a.slots >= b.slots && a.k_pad >= b.k_pad && a.seg_points >= b.seg_points && a.grid_points >= b.grid_points &&
           a.large_points >= b.large_points && a.large_chunks >= b.large_chunks && a.large_starts >= b.large_starts && a.large_clouds >= b.large_clouds;
}

static void check_workspace()
{
    // the rounding rule and the per-cloud shares
    EXPECT(kFpsWsAlign == 256 && fps_ws_up(0) == 0 && fps_ws_up(1) == 256 && fps_ws_up(256) == 256 && fps_ws_up(257) == 512);
    EXPECT(fps_k_pad(1) == 64 && fps_k_pad(64) == 64 && fps_k_pad(65) == 128 && fps_k_pad(20000) == 20032);
    EXPECT(fps_grid_points(1) == 64 && fps_grid_points(64) == 64 && fps_grid_points(24576) == 24576 && fps_grid_points(24001) == 24064);
    EXPECT(fps_seg_points(1000, kFpsGrid) == 1000 && fps_seg_points(1000, kFpsMulti) == 1000 && fps_seg_points(1000, kFpsLarge) == 0);
    // monotone in every n (within its sampler's range) and every k, one cloud of each sampler
    const int lo[3] = {1, kFpsGridMaxN + 1, kFpsMultiMaxN + 1}, hi[3] = {kFpsGridMaxN, kFpsMultiMaxN, kFpsLargeMaxN};
    for (int which = 0; which < 3; which++) {
        int n[3] = {1000, 30000, 300000}, k[3] = {100, 100, 100};
        n[which] = lo[which];
        FpsWorkspace prev = workspace_of(3, n, k, 0, false);
        for (int v = lo[which]; v <= hi[which]; v += (v < lo[which] + 3000 || v > hi[which] - 3000) ? 1 : 211) {
            n[which] = v;
            const FpsWorkspace w = workspace_of(3, n, k, 0, false);
            EXPECT(no_less(w, prev));
            prev = w;
        }
        n[which] = hi[which];
        prev = workspace_of(3, n, k, 0, false);
        for (int v = 100; v <= 70000 && v <= n[which]; v++) {
            k[which] = v;
            const FpsWorkspace w = workspace_of(3, n, k, 0, false);
            EXPECT(no_less(w, prev) && w.k_pad >= (size_t)(k[0] + k[1] + k[2]));
            prev = w;
        }
    }
    // the counts themselves at one call
    {
        const int n[3] = {1000, 30000, 300000}, k[3] = {100, 129, 64};
        const FpsWorkspace w = workspace_of(3, n, k, 0, false);
        EXPECT(w.slots == 2 * 64 && w.k_pad == 128 + 192 + 64 && w.seg_points == 31000 && w.grid_points == 1024);
        EXPECT(w.large_points == (size_t)fps_plan(300000, 0).npad && w.large_chunks == (size_t)fps_plan(300000, 0).chunks);
        EXPECT(w.large_starts == (size_t)fps_plan(300000, 0).starts && w.large_clouds == 1);
    }
    // nothing for a sampler without a cloud in the call
    {
        const int n[2] = {1000, 24576}, k[2] = {10, 20000};
        FpsWorkspace w = workspace_of(2, n, k, 0, false);
        EXPECT(w.slots == 0 && w.large_points == 0 && w.large_chunks == 0 && w.large_starts == 0 && w.large_clouds == 0);
        EXPECT(w.grid_points == 1024 + 24576 && w.seg_points == 25576);
        w = workspace_of(2, n, k, 0, true);
        EXPECT(w.grid_points == 0 && w.slots == 2 * (6 + 64) && w.large_points == 0 && w.large_clouds == 0 && w.seg_points == 25576);
        w = workspace_of(2, n, k, 1, false);
        EXPECT(w.grid_points == 0 && w.slots == 0 && w.seg_points == 0 && w.large_clouds == 2 && w.large_points == 1024 + 24576);
        const int m[2] = {24577, 262144};
        w = workspace_of(2, m, k, 0, false);
        EXPECT(w.grid_points == 0 && w.slots == 2 * (64 + 64) && w.large_points == 0 && w.large_clouds == 0);
    }
    // a deferred check's buffer: whole lines, nothing overlaps, and the total is the pieces' sum
    for (int trial = 0; trial < 2000; trial++) {
        int n[kFMaxJobs], k[kFMaxJobs];
        const int nj = 1 + rnd(kFMaxJobs);
        size_t points = 0, sum = kFpsWsAlign;
        for (int q = 0; q < nj; q++) {
            n[q] = 1 + rnd(trial & 1 ? 300 : kFpsGridMaxN);
            k[q] = 1 + rnd(n[q]);
        }
        const FpsDeferredLayout l = fps_deferred_layout(nj, n, k);
        size_t end = kFMaxJobs * sizeof(int);          // the verdict words
        for (int q = 0; q < nj; q++) {
            EXPECT(l.xyz[q] % kFpsWsAlign == 0 && l.out[q] % kFpsWsAlign == 0 && l.pdist[q] % kFpsWsAlign == 0);
            EXPECT(l.xyz[q] >= end && l.out[q] >= l.xyz[q] + (size_t)n[q] * 12 && l.pdist[q] >= l.out[q] + (size_t)k[q] * 4);
            end = l.pdist[q] + (size_t)k[q] * 4;
            EXPECT(l.segoff[q] == (int)points);
            points += (size_t)n[q];
            sum += fps_ws_up((size_t)n[q] * 12) + 2 * fps_ws_up((size_t)k[q] * 4);
        }
        EXPECT(l.segmin % kFpsWsAlign == 0 && l.segmin >= end && l.bytes >= l.segmin + points * kFVMaxSeg * sizeof(float));
        EXPECT(l.bytes == sum + fps_ws_up(points * kFVMaxSeg * sizeof(float)) && l.bytes % kFpsWsAlign == 0);
    }
}

int main(int argc, char **argv)
{
    // with arguments: print the plan of (n, force_large) as genpc_fps_plan lays it out (the Python side compares)
    if (argc == 3) {
        const FpsPlan p = fps_plan(atoi(argv[1]), atoi(argv[2]));
        printf("%d %d %d %d %d %d %d %d\n", p.sampler, p.cells_max, p.cells_target, p.npad, p.chunks, p.starts, p.lds_bytes, p.build_own);
        return 0;
    }
    // the three ranges and their boundaries
    EXPECT(fps_plan(1, 0).sampler == kFpsGrid);
    EXPECT(fps_plan(24576, 0).sampler == kFpsGrid);
    EXPECT(fps_plan(24577, 0).sampler == kFpsMulti);
    EXPECT(fps_plan(262144, 0).sampler == kFpsMulti);
    EXPECT(fps_plan(262145, 0).sampler == kFpsLarge);
    EXPECT(fps_plan(4194304, 0).sampler == kFpsLarge);
    EXPECT(kFpsGridMaxN == 24576 && kFpsMultiMaxN == 262144 && kFpsLargeMaxN == 4194304);
    // nothing but the sampler for the two that size themselves
    for (int n : {1, 24576, 24577, 262144}) {
        const FpsPlan p = fps_plan(n, 0);
        EXPECT(p.cells_max == 0 && p.cells_target == 0 && p.npad == 0 && p.chunks == 0 && p.starts == 0 && p.lds_bytes == 0);
    }
    // force_large: any size
    for (int n : {1, 2, 63, 24576, 24577, 262144, 262145, 4194304}) {
        const FpsPlan p = fps_plan(n, 1);
        EXPECT(p.sampler == kFpsLarge);
        EXPECT(p.npad >= n && p.npad % kFpsLargePad == 0 && p.npad - n < kFpsLargePad);
        EXPECT(p.chunks * kFpsLargeChunk == p.npad && p.chunks % 4 == 0);
        EXPECT(p.cells_target >= 1 && p.cells_target <= p.cells_max && p.starts == p.cells_max + 1);
        EXPECT(p.lds_bytes == (int)kFpsLargeLdsBytes && p.lds_bytes <= 64 * 1024 && p.build_own == 0);
    }
    EXPECT(fps_plan(1, 1).npad == 128 && fps_plan(1, 1).chunks == 16 && fps_plan(1, 1).cells_target == 64);
    EXPECT(fps_plan(262145, 0).npad == 262272 && fps_plan(262145, 0).cells_target == 12288);
    // refusals
    for (int force = 0; force < 2; force++) {
        EXPECT(fps_plan(0, force).sampler == kFpsNone);
        EXPECT(fps_plan(-5, force).sampler == kFpsNone);
        EXPECT(fps_plan(4194305, force).sampler == kFpsNone);
        EXPECT(fps_plan(2147483647, force).sampler == kFpsNone);
        EXPECT(fps_plan(4194305, force).npad == 0 && fps_plan(4194305, force).lds_bytes == 0);
    }
    // every workspace count is monotone in n (every n near a boundary of the padding, strides elsewhere)
    FpsPlan prev = fps_plan(1, 1);
    for (int n = 2; n <= kFpsLargeMaxN; n += (n < 70000 || n > kFpsLargeMaxN - 70000) ? 1 : 997) {
        const FpsPlan p = fps_plan(n, 1);
        EXPECT(p.npad >= prev.npad && p.chunks >= prev.chunks && p.cells_target >= prev.cells_target && p.cells_max >= prev.cells_max);
        EXPECT(p.starts >= prev.starts && p.lds_bytes >= prev.lds_bytes);
        if (g_fail) break;
        prev = p;
    }
    // every packed field holds its maximum at the limit
    {
        const FpsPlan p = fps_plan(kFpsLargeMaxN, 1);
        const unsigned long long last_pos = (unsigned long long)p.npad - 1, last_index = (unsigned long long)kFpsLargeMaxN - 1;
        EXPECT(last_pos < (1ull << kFpsLargePosBits));
        EXPECT(last_index < (1ull << kFpsLargeIndexBits));
        const unsigned long long key = (last_index << kFpsLargePosBits) | last_pos;
        EXPECT((key >> kFpsLargePosBits) == last_index && (key & ((1ull << kFpsLargePosBits) - 1)) == last_pos);
        EXPECT((long long)key >= 0);
        const unsigned last_cell = (unsigned)p.cells_max - 1, last_sample = (unsigned)kFpsLargePick - 1;
        const unsigned long long item = ((unsigned long long)last_sample << kFpsLargeCellBits) | last_cell;
        EXPECT(item <= 0xffffffffull);
        EXPECT((unsigned)(item >> kFpsLargeCellBits) == last_sample && ((unsigned)item & ((1u << kFpsLargeCellBits) - 1u)) == last_cell);
        EXPECT((long long)p.npad * 16 < (1ll << 31) * 16 && (long long)p.chunks * 4 == p.npad / 2);
        EXPECT(p.cells_max < (1 << 19));
    }
    check_classes();
    check_multi_shape();
    check_multi_launches();
    check_verify_segments();
    check_workspace();
    if (g_fail) return 1;
    printf("fps_plan_check: ok\n");
    return 0;
}
