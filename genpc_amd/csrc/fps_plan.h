// fps_plan.h -- every host decision of a farthest-point-sampling call, as pure functions.
// fps_plan: which sampler a cloud takes, decided from its point count alone, and for the large sampler (fps_large.hip) every size
// the call needs: the grid's cell budget, the element count of each workspace piece, the widths of its packed fields and its LDS
// bytes.  fps_grid_takes (fps_grid.hip), fps_call (fps_call.hip) and fps_large.hip read it and decide nothing besides.
//   up to kFpsGridMaxN points    the one-workgroup sampler with its running minima in LDS (fps_grid.hip: fps_grid_kernel), unless
//                                genpc_fps_tune(256) sends the cloud to the multi-workgroup kernel -- the caller applies that hook
//   up to kFpsMultiMaxN points   the multi-workgroup kernel (fps.hip: fps_kernel)
//   up to kFpsLargeMaxN points   the one-workgroup sampler with its running minima in global memory (fps_large.hip), which also
//                                takes any smaller cloud when it is asked for by name (genpc_fps_large: force_large)
// The rest of a call (second half of this header; fps_call carries it out): the register class of fps_kernel a launch takes
// (kFpsClassPoints, stated here alone), the co-residency shape of a cloud on the device as FpsDevice describes it
// (fps_multi_shape), the grouping of clouds into launches with their hand-off slots and admission units (fps_multi_launches), the
// segments of the verification (fps_verify_segments), the element counts of the workspace (fps_workspace) and the bytes of a
// deferred check's private buffer (fps_deferred_layout).
// Host code only, no HIP: a plain C++ program can include it (tests/fps_plan_check.cpp does); the library exports fps_plan as
// genpc_fps_plan.
#pragma once
#include <stddef.h>

namespace genpc {

constexpr int kFpsGridMaxN = 24576;           // fps_grid_kernel: 4 B of LDS per point (+ 0.5 per point of chunk maxima)
constexpr int kFpsMultiMaxN = 262144;         // fps_kernel: 64 workgroups x 192 threads x 24 points in registers and more
constexpr int kFpsLargeMaxN = 4194304;        // fps_large_kernel: what its packed fields hold (below)

enum FpsSampler : int { kFpsNone = -1, kFpsGrid = 0, kFpsMulti = 1, kFpsLarge = 2 };

// ---- the large sampler's constants
constexpr int kFpsLargeThreads = 1024;        // one workgroup per cloud
constexpr int kFpsLargeCand = 128;            // candidates a round lists
constexpr int kFpsLargePick = 64;             // samples a round draws at most
constexpr int kFpsLargeChunk = 8;             // points per chunk: one upper bound of their running minima per chunk
constexpr int kFpsLargePad = 128;             // a cloud's running minima are padded to this many points (16 chunks: whole 64-byte rows of chunk maxima)
// The grid is grid.hip's launch_cell_grid_build as it stands (fps_large.hip asserts kFpsLargeCellsMax against the build's
// LDS budget, kCellGridMaxCells): at most 15360 cells, about one per 16 points of the bounding box's volume -- surfaces fill a
// fraction of the cells, and a cell of the cloud then holds a few chunks.
constexpr int kFpsLargeCellsMax = 15360;
constexpr int kFpsLargeCellsTargetMax = 12288, kFpsLargeCellsTargetMin = 64, kFpsLargePointsPerCell = 16;
// packed fields.  An update's work item is (sample of the round << kFpsLargeCellBits | cell); a tied point's key on the tie path
// is (original index << kFpsLargePosBits | position in cell order), 64 bits wide.
constexpr int kFpsLargeCellBits = 14;
constexpr int kFpsLargeSampleBits = 6;
constexpr int kFpsLargePosBits = 22;
constexpr int kFpsLargeIndexBits = 22;        // (also the steps of the tie path's bisection over original indices)
static_assert(kFpsLargeCellsMax <= (1 << kFpsLargeCellBits), "a work item holds every cell");
static_assert(kFpsLargePick <= (1 << kFpsLargeSampleBits), "a work item holds every sample of a round");
static_assert(kFpsLargeCellBits + kFpsLargeSampleBits <= 32, "a work item is 32 bits");
static_assert(kFpsLargeMaxN <= (1 << kFpsLargePosBits), "a key holds every position");
static_assert(kFpsLargeMaxN <= (1 << kFpsLargeIndexBits), "a key holds every original index");
static_assert(kFpsLargePosBits + kFpsLargeIndexBits <= 63, "a key is a non-negative 64-bit number");
static_assert(kFpsLargeCellsMax < (1 << 19), "the update's division of a cell number by reciprocal is exact below 2^19");
static_assert(kFpsLargePad % (2 * kFpsLargeChunk) == 0 && kFpsLargePad / kFpsLargeChunk % 4 == 0, "chunk maxima are read four at a time");
// LDS: the queue (work items with their cell-to-sample bounds, 8 bytes each; the tie path's keys share it), the round's lists
// (fps_large.hip names the pieces) and the shared scalars
constexpr int kFpsLargeQueue = 4096;          // work items of an update / tied points of the tie path
constexpr int kFpsLargeListFloats = 1792;     // candidates, samples, reduction scratch, scalars (fps_grid_kernel's layout)
constexpr int kFpsLargeRangeInts = 6 * kFpsLargePick;      // the cell range of every sample's ball: first cell and width per axis
constexpr size_t kFpsLargeLdsBytes = (size_t)kFpsLargeQueue * 8 + (size_t)kFpsLargeListFloats * 4 + (size_t)kFpsLargeRangeInts * 4;
static_assert(kFpsLargeLdsBytes <= 64 * 1024, "no opt-in needed for the dynamic LDS of the launch");

struct FpsPlan {
    int sampler;            // FpsSampler; kFpsNone: the call is refused (n < 1 or n > kFpsLargeMaxN)
    // the rest is 0 unless sampler == kFpsLarge
    int cells_max;          // cells of the grid at most (the cell table has cells_max + 1 entries)
    int cells_target;       // cells asked of the bounding box
    int npad;               // running minima (4 B each) and sorted points (16 B each): n rounded up to kFpsLargePad
    int chunks;             // chunk maxima (4 B each): npad / kFpsLargeChunk
    int starts;             // entries of the cell table: cells_max + 1
    int lds_bytes;          // dynamic LDS of the launch
    int build_own;          // 0: the grid is built by launch_cell_grid_build as it stands; (1: a build of the sampler's own -- not used)
};

inline FpsPlan fps_plan(int n, int force_large)
{
    FpsPlan p{kFpsNone, 0, 0, 0, 0, 0, 0, 0};
    if (n < 1 || n > kFpsLargeMaxN) return p;
    if (!force_large && n <= kFpsGridMaxN) { p.sampler = kFpsGrid; return p; }
    if (!force_large && n <= kFpsMultiMaxN) { p.sampler = kFpsMulti; return p; }
    p.sampler = kFpsLarge;
    p.cells_max = kFpsLargeCellsMax;
    int target = n / kFpsLargePointsPerCell;
    target = target < kFpsLargeCellsTargetMin ? kFpsLargeCellsTargetMin : target;
    p.cells_target = target > kFpsLargeCellsTargetMax ? kFpsLargeCellsTargetMax : target;
    p.npad = (int)(((long long)n + kFpsLargePad - 1) / kFpsLargePad * kFpsLargePad);
    p.chunks = p.npad / kFpsLargeChunk;
    p.starts = p.cells_max + 1;
    p.lds_bytes = (int)kFpsLargeLdsBytes;
    p.build_own = 0;
    return p;
}

// ---- the multi-workgroup kernel (fps.hip) and the verification (fps_verify.hip): what a call decides about them
constexpr int kFThreads = 192;           // worker threads of a workgroup: three waves, the fourth wave coordinates -- one wave per SIMD
constexpr int kFMaxR = 24;               // points a thread keeps in registers at most
constexpr int kFMaxW = 64;               // workgroups of a cloud at most (a lane of the polling wave per workgroup)
constexpr int kFMaxJobs = 8;             // clouds of one launch, of one verification
constexpr int kFPointsPerWg = 192;       // target: one point per worker thread.  What a round yields grows with the NUMBER of lists
                                         // (64 lists x 4 candidates: ~45 samples per exchange; 8 lists: 13), so small clouds are spread
                                         // over many workgroups too; the cap of 64 workgroups raises the share for clouds beyond 16384 points
constexpr int kFVBlock = 128;            // threads (points) of a verification block
constexpr int kFVMaxSeg = 16;            // segments the verification cuts a sample list into at most

// The register classes of fps_kernel<FMA, R>: a launch whose clouds keep up to R points per thread takes the first class that
// holds them.  Stated HERE ALONE: fps.hip builds its one table of instantiations from kFpsClassPoints and both launches and asks
// the runtime for the occupancy through that table, indexed by fps_class.  A launch is sized from the occupancy of the
// instantiation it takes; were the two to disagree, the launch would not be co-resident and the hand-off would spin to its timeout.
constexpr int kFpsClasses = 6;
constexpr int kFpsClassPoints[kFpsClasses] = {2, 4, 8, 12, 16, 24};
static_assert(kFpsClassPoints[kFpsClasses - 1] == kFMaxR, "the last class holds every R a shape can have");
inline int fps_class(int R)
{
    int cls = 0;
    while (cls < kFpsClasses - 1 && R > kFpsClassPoints[cls]) cls++;
    return cls;
}

// The device as the plan sees it.  All workgroups of a launch must be resident together (they wait for each other), so what
// counts is what THIS device holds of the instantiation a launch takes: a partitioned or smaller part has fewer than the 256 CUs
// of a full MI355X.  Another stream's kernels are not counted -- a hand-off that times out because of them is retried one cloud at
// a time by genpc_amd/fps.py.
struct FpsDevice {
    int cus;                                 // compute units, >= 1
    int blocks_per_cu[kFpsClasses];          // workgroups of each class one CU holds at a time, as the runtime reports it: >= 1
};
inline int fps_budget(const FpsDevice &dev, int R) { return dev.blocks_per_cu[fps_class(R)] * dev.cus; }

// A cloud's shape on the multi-workgroup kernel: as many workgroups as its size asks for, fewer (more points per thread) if the
// device does not hold them.  !ok: no number of workgroups the device holds keeps the points within kFMaxR per thread -- the call
// is refused ("needs more co-resident workgroups").  Fewer workgroups mean a larger R, a larger R may mean a class of which the
// device holds fewer: hence a loop; it ends at W == 1 at the latest (a budget is at least 1).
struct FpsShape {
    bool ok;
    int W, R;          // workgroups; points per thread
};
inline FpsShape fps_multi_shape(int n, const FpsDevice &dev)
{
    int W = (n + kFPointsPerWg - 1) / kFPointsPerWg;
    W = W > kFMaxW ? kFMaxW : (W < 1 ? 1 : W);
    for (;;) {
        const int R = ((n + W - 1) / W + kFThreads - 1) / kFThreads;
        if (R > kFMaxR) return {false, W, R};
        const int budget = fps_budget(dev, R);
        if (W <= budget || W == 1) return {W <= budget, W, R};
        W = W > 2 * budget ? budget : W - 1;
    }
}

// The launches of a call's multi-workgroup clouds, shape[0 .. cb) in call order.  A launch takes up to kFMaxJobs consecutive
// clouds; its grid is (largest W) x (clouds) workgroups of the class of the largest R, all of it resident together, so a further
// cloud joins only while that grid stays within the budget.  The hand-off slots are per (cloud, step parity, workgroup): cloud q's
// are slot0[q] .. slot0[q] + 2 W, numbered through all launches.
// units: the hand-off needs the launch resident as a whole, like the one-launch auction (emd_auction.hip): both take their share of
// the chip from one budget in quarter-CU units -- a workgroup of an instantiation the CU holds k of costs ceil(4 / k) -- so two such
// launches of different streams never sit half-resident waiting for workgroups the other one keeps out (two samplings of
// different lanes could spin against each other until the timeout).
struct FpsLaunch {
    int first, count;          // its clouds: shape[first .. first + count)
    int wmax, rmax;            // grid wmax x count, instantiation fps_class(rmax)
    int units;                 // for persist_reserve
};
// launches[] and slot0[] have room for cb entries; returns the number of launches
inline int fps_multi_launches(int cb, const FpsShape *shape, const FpsDevice &dev, FpsLaunch *launches, int *slot0)
{
    int nl = 0, slot = 0;
    for (int first = 0; first < cb;) {
        FpsLaunch l = {first, 0, 0, 1, 0};
        while (first + l.count < cb && l.count < kFMaxJobs) {
            const FpsShape &s = shape[first + l.count];
            const int wm = s.W > l.wmax ? s.W : l.wmax, rm = s.R > l.rmax ? s.R : l.rmax;
            if (l.count > 0 && (long long)wm * (l.count + 1) > fps_budget(dev, rm)) break;
            slot0[first + l.count] = slot;
            slot += 2 * s.W;
            l.wmax = wm;
            l.rmax = rm;
            l.count++;
        }
        const int per_cu = dev.blocks_per_cu[fps_class(l.rmax)];
        l.units = l.wmax * l.count * ((4 + per_cu - 1) / per_cu);
        launches[nl++] = l;
        first += l.count;
    }
    return nl;
}

// Segments (grid.z) the verification of nj clouds, the largest of nmax points, cuts its sample lists into: about four blocks per
// CU.  single: the clouds are the large sampler's -- no segment minima are reserved for them (fps_seg_points), and their point
// blocks fill the chip anyway.
inline int fps_verify_segments(int nmax, int nj, int cus, bool single)
{
    if (single) return 1;
    const int blocks = (nmax + kFVBlock - 1) / kFVBlock * nj;
    const int nseg = (4 * cus) / (blocks > 0 ? blocks : 1);
    return nseg < 1 ? 1 : (nseg > kFVMaxSeg ? kFVMaxSeg : nseg);
}

// ---- the workspace.  kFpsWsAlign is the rounding rule of the library's scratch (ws_layout.h: WsLayout::up; fps.h asserts that
// the two agree): a piece starts on a 256-byte boundary and takes its size rounded up to 256 bytes.
constexpr size_t kFpsWsAlign = 256;
inline size_t fps_ws_up(size_t bytes) { return (bytes + kFpsWsAlign - 1) / kFpsWsAlign * kFpsWsAlign; }
// a cloud's share of three pieces: its samples' recorded minima (k floats in whole lines), its rows of segment minima (one per
// point; none for a cloud of the large sampler, whose check is never cut), its points in cell order for the grid sampler
inline size_t fps_k_pad(int k) { return fps_ws_up((size_t)k * sizeof(float)) / sizeof(float); }
inline size_t fps_seg_points(int n, int sampler) { return sampler == kFpsLarge ? (size_t)0 : (size_t)n; }
inline size_t fps_grid_points(int n) { return ((size_t)n + 63) & ~(size_t)63; }

// Element counts of a call's workspace pieces (beside the 64-word status block and one verdict word per cloud).  sampler[j]: the
// FpsSampler cloud j takes IN THIS CALL (fps_plan's answer with the genpc_fps_tune hook applied); shape[0 .. cb): the shapes of the
// clouds with sampler[j] == kFpsMulti, in call order.  A call without a cloud of a sampler reserves nothing for it.
struct FpsWorkspace {
    size_t slots;              // hand-off slots of the multi-workgroup clouds: 2 W each
    size_t k_pad;              // recorded minima: every cloud
    size_t seg_points;         // points with rows of segment minima (x kFVMaxSeg floats)
    size_t grid_points;        // float4 per point: the grid sampler's clouds
    size_t large_points, large_chunks, large_starts, large_clouds;          // the large sampler's pieces, as fps_plan counts them
};
inline FpsWorkspace fps_workspace(int c, const int *n, const int *k, const int *sampler, int cb, const FpsShape *shape)
{
    FpsWorkspace w = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int q = 0; q < cb; q++) w.slots += 2 * (size_t)shape[q].W;
    for (int j = 0; j < c; j++) {
        w.k_pad += fps_k_pad(k[j]);
        w.seg_points += fps_seg_points(n[j], sampler[j]);
        if (sampler[j] == kFpsGrid) w.grid_points += fps_grid_points(n[j]);
        if (sampler[j] == kFpsLarge) {
            const FpsPlan p = fps_plan(n[j], 1);
            w.large_points += (size_t)p.npad;
            w.large_chunks += (size_t)p.chunks;
            w.large_starts += (size_t)p.starts;
            w.large_clouds++;
        }
    }
    return w;
}

// A deferred check's private buffer (fps_verify.hip; not the pool's): the verdict words' line, three copies per cloud -- points,
// samples, recorded minima -- and the segment minima of all clouds.  Byte offsets from the buffer's start.
static_assert(kFMaxJobs * sizeof(int) <= kFpsWsAlign, "the verdict words share the first line");
struct FpsDeferredLayout {
    size_t bytes;
    size_t xyz[kFMaxJobs], out[kFMaxJobs], pdist[kFMaxJobs], segmin;
    int segoff[kFMaxJobs];          // the cloud's first point in the segment minima
};
inline FpsDeferredLayout fps_deferred_layout(int nj, const int *n, const int *k)
{
    FpsDeferredLayout l = {};
    size_t off = kFpsWsAlign, points = 0;
    for (int q = 0; q < nj; q++) {
        l.xyz[q] = off;
        off += fps_ws_up((size_t)n[q] * 3 * sizeof(float));
        l.out[q] = off;
        off += fps_ws_up((size_t)k[q] * sizeof(int));
        l.pdist[q] = off;
        off += fps_ws_up((size_t)k[q] * sizeof(float));
        l.segoff[q] = (int)points;
        points += (size_t)n[q];
    }
    l.segmin = off;
    l.bytes = off + fps_ws_up(points * kFVMaxSeg * sizeof(float));
    return l;
}

}  // namespace genpc
