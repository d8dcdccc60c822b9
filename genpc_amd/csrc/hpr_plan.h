// hpr_plan.h -- the plan of one hidden-point-removal call (hpr.hip hpr_run, behind genpc_hpr_visibility and
// genpc_hpr_best_view_counts): the form of the call (one kernel or two), what the first kernel takes before it hands a point
// over, the sort's key bits, the size of the polygon stores, every grid and the element count of every piece of the workspace.
// hpr_run and the launchers of the hpr_*.hip files read the plan and decide nothing besides; the measured numbers behind every
// threshold stand beside it here (they are the history of the choice, not today's timings: DESIGN.md section 4.6).
// Host code only, no HIP: a plain C++ program can include it (tests/hpr_plan_check.cpp does); the library exports the function
// as genpc_hpr_plan, and tests/test_gpu_hpr_forms.py asks that call which shapes reach which form.
#pragma once
#include <algorithm>

namespace genpc {

constexpr int kHprThreads = 128;
constexpr int kHprMaxV = 10;            // polygon vertices per thread in LDS (20 KB per 128-thread block).  Round 2: 24 -> 16 (24.7 -> 20.9 ms at 64 x 10000; 12 then lost: too many points fell to a second pass that held five waves per CU).  With the second pass's 4 KiB tier the balance moved: 1024 x 10000 blob / scan 83.7 / 51.4 ms at 16, 68.5 / 43.1 at 12, 66.2 / 41.9 at 10, 75.4 / 43.3 at 9, 99 / 52 at 8
constexpr int kHprOverCap = 1024;       // vertices per polygon in the second pass (2 x 16 KB of LDS per wave)
constexpr int kHprRimTiles = 256;       // clouds of at least this many tiles: one-kernel form, silhouette points handed to the second pass
constexpr int kHprWorkLine = 32, kHprWorkWords = 16 * kHprWorkLine;      // the passes' work counters: a 128-byte line each
constexpr int kHprStatusWords = 64;     // the 256-byte header (hpr.h: HprStatus)
// one-wave blocks per CU: the parked points' first try, the wave-per-point pass (128-vertex tier: 4 KiB of LDS per wave), its
// kHprOverCap tier (two 16 KiB buffers per wave)
constexpr int kHprDecideWaves = 64, kHprWalkWaves = 40, kHprLargeWaves = 5;
constexpr long long kHprGlobalBytes = 256ll << 20;      // the global-polygon tier's buffers, at most

// GENPC_HPR_NOCULL, a mask of alternative paths (results unchanged; tests/test_gpu_hpr_paths.py runs both)
enum HprNoCull : int {
    kHprNoRounds = 128,         // no decisions without the walk in the wave-per-point pass
    kHprBlockVerify = 512,      // two-kernel form WITH the first kernel's own verify phase
};

struct HprAsk {
    int c = 0, n = 0;              // views, points
    int best_only = 0;             // genpc_hpr_best_view_counts
    int cus = 256;                 // compute units of the device
    // the switches, as given
    int env_split = -1;            // GENPC_HPR_SPLIT: 1 two-kernel form, 0 one kernel, < 0 by size
    int env_park_mb = 3072;        // GENPC_HPR_PARK_MB (<= 0 counts as 1)
    int env_home_tiles = 1;        // GENPC_HPR_HOME_TILES, clamped to 1 .. 3
    int env_home_chunks = 2;       // GENPC_HPR_HOME_CHUNKS, clamped to 1 .. 4
    int env_decide_kernel = 1;     // GENPC_HPR_DECIDE_KERNEL
    int no_cull = 0;               // GENPC_HPR_NOCULL
};

struct HprPlan {
    bool too_large;                // more than 4096 views or 2^31 - 1 (view, point) pairs: the call fails
    int ntiles;                    // tiles of kHprThreads consecutive positions per view
    int split;                     // two-kernel form
    bool prune;                    // views that cannot be the best any more are dropped after the first polygon kernel
    int key_bits;                  // of the view sort
    int max_clips;                 // clips after which a polygon goes to the wave-per-point pass
    int home_tiles, home_chunks;   // what the first kernel clips by before it tries to verify / parks: tiles, 32-candidate chunks of the first
    int chunk_w;                   // first kernel: candidates marked at a time against the polygon as the previous ones left it
    int straggle_from, straggle_lanes;      // the first kernel hands a block's undecided points over from this tile batch on, when at most so many are left
    long long park_cap, park_bytes;         // the polygon store: parked points it holds (0: no store), bytes
    bool decide_kernel;            // the parked points' first try in a kernel of its own
    // grids
    int row_grid, bounds_grid;     // 256-thread blocks over the points; the same, capped (the bounds kernel strides)
    int view_grid;                 // 256-thread blocks over the views
    int decide_blocks, walk_blocks, large_blocks;      // one-wave blocks of the wave-per-point passes (decide: a multiple of 8)
    int global_blocks, gcap;       // the global-polygon tier: blocks, vertices per buffer
    long long global_bytes;
    // element counts of the workspace's pieces (the sort's scratch is rocprim's to size)
    long long pairs;               // views x points: list, keys, indices, hard, hardlist
    long long fl_count;            // flipped points: doubles
    long long tile_count;          // tile records
    long long surv_count;          // parked points' records (0: one-kernel form)
};

inline HprPlan hpr_plan(const HprAsk &a)
{
    HprPlan p{};
    const long long total = (long long)a.c * a.n;
    p.too_large = a.c > 4096 || total > 0x7fffffffll || a.n > 0x7fffffff - 8;      // (the last: gcap below is an int)
    if (p.too_large || a.c <= 0 || a.n <= 0) return p;
    auto blocks_of = [](long long items, int per) { return (int)((items + per - 1) / per); };
    p.ntiles = blocks_of(a.n, kHprThreads);
    // Split form (the first kernel stops after the home tiles + verification and saves the undecided points' polygons; a
    // wave per point continues from them): for clouds of < 256 tiles.  Round 3, first half: only for >= 4 M (view, point)
    // pairs, with a dense one-thread-per-survivor second kernel (1024 x 10000: 128 -> 88 ms; 64 x 10000 14.3 -> 16.6).  With
    // the wave-per-point continuation: 1024 x 10000 64 / 39 / 44 -> 58.6 / 32 / 37.5 ms (blob / two scans), 64 x 10000
    // 7.3 -> 6.9.  A few views of a large cloud keep the one-kernel form (2 x 165546: 14.9 against 17.8 ms): there the lanes
    // of a block want the same tiles, and staging them once per block through LDS beats per-wave reads
    // (GENPC_HPR_SPLIT=0/1 overrides).
    p.split = a.env_split >= 0 ? a.env_split : (p.ntiles < kHprRimTiles && total >= 100000ll ? 1 : 0);
    // best_only (viewpoint_select): views are only dropped in the two-kernel form
    p.prune = a.best_only && p.split;
    p.key_bits = 20;               // view << 20 | Morton code
    while ((1 << (p.key_bits - 20)) < a.c) p.key_bits++;
    // clips after which a polygon goes to the wave-per-point pass (large clouds: 96 -- 2 x 165546 points 46 -> 40 ms; many
    // views of a small cloud: the second pass fills up instead -- 1024 x 10000 points 154 ms with 256, 168 with 128, 180
    // with 96; large clouds: 96 -> 48 once the wave-per-point pass clipped by all lanes: 2 x 165546 24.9 -> 21.5 ms)
    p.max_clips = p.ntiles >= kHprRimTiles ? 48 : 256;
    // The undecided points' polygons: at most one per point the accept pass left over.  That count stays on the device
    // (round 4 fetched it to size the store, the first of six stream synchronisations of this entry point): the store is
    // sized for every (view, point) pair up to GENPC_HPR_PARK_MB, and a point whose slot would lie beyond it is listed
    // for the wave-per-point pass instead of parked (it restarts from the box there: same result, computed again).
    const long long poly_bytes = (long long)kHprMaxV * 16;          // kHprMaxV double2
    const long long park_mb = a.env_park_mb > 0 ? a.env_park_mb : 1;
    p.park_cap = p.split ? std::min(total, std::max(1ll, (park_mb << 20) / poly_bytes)) : 0;
    p.park_bytes = p.park_cap * poly_bytes;
    // the first kernel hands a block's undecided points over after 4 tile batches, all of them (see the kernel)
    p.straggle_from = 4;
    p.straggle_lanes = kHprThreads;
    p.chunk_w = 32;
    // split form: home tiles (the point's own, the next, the previous) the first kernel takes before it tries to verify and
    // parks what is left; the wave-per-point pass decides most parked points from the polygon they bring and takes the
    // remaining home tiles only for the others
    p.home_tiles = p.split ? std::min(std::max(a.env_home_tiles, 1), 3) : 3;
    p.home_chunks = p.split && p.home_tiles == 1 ? std::min(std::max(a.env_home_chunks, 1), 4) : 4;
    p.decide_kernel = p.split && a.env_decide_kernel && !(a.no_cull & kHprNoRounds);
    p.row_grid = blocks_of(a.n, 256);
    p.bounds_grid = std::min(p.row_grid, 1024);
    p.view_grid = blocks_of(a.c, 256);
    // The wave-per-point passes.  How many points each of them finds is known on the device only: every pass is a fixed
    // grid of one-wave blocks -- as many as the chip holds of that kernel, or as there can be items -- that reads its count
    // from the status header and leaves at once when it is zero (an empty pass costs its launch, ~5 us).
    auto grid_of = [&](int per_cu) { return (int)std::min(total, (long long)per_cu * a.cus); };
    p.decide_blocks = (grid_of(kHprDecideWaves) + 7) & ~7;          // block b -> segment b % 8
    p.walk_blocks = grid_of(kHprWalkWaves);
    p.large_blocks = grid_of(kHprLargeWaves);
    // polygons over 1024 vertices (exactly co-spherical input, lattices seen from their centre): a third tier with the
    // polygon in global memory, n + 8 vertices per buffer -- it cannot overflow -- a pair of buffers per wave of the grid
    p.gcap = a.n + 8;
    const long long per = 2ll * p.gcap * 16;
    p.global_blocks = (int)std::min(std::min(total, 1024ll), std::max(1ll, kHprGlobalBytes / per));
    p.global_bytes = p.global_blocks * per;
    p.pairs = total;
    p.fl_count = total * 3;
    p.tile_count = (long long)a.c * p.ntiles;
    p.surv_count = p.split ? total : 0;
    return p;
}

}  // namespace genpc
