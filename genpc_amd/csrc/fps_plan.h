// fps_plan.h -- which sampler a cloud of a farthest-point-sampling call takes, decided from its point count alone, and for the
// large sampler (fps_large.hip) every size the call needs: the grid's cell budget, the element count of each workspace piece, the
// widths of its packed fields and its LDS bytes.  fps_grid_takes (fps_grid.hip), the entry points of fps.hip and fps_large.hip read
// this header and decide nothing besides.
//   up to kFpsGridMaxN points    the one-workgroup sampler with its running minima in LDS (fps_grid.hip: fps_grid_kernel), unless
//                                genpc_fps_tune(256) sends the cloud to the multi-workgroup kernel -- the caller applies that hook
//   up to kFpsMultiMaxN points   the multi-workgroup kernel (fps.hip: fps_kernel)
//   up to kFpsLargeMaxN points   the one-workgroup sampler with its running minima in global memory (fps_large.hip), which also
//                                takes any smaller cloud when it is asked for by name (genpc_fps_large: force_large)
// Host code only, no HIP: a plain C++ program can include it (tests/fps_plan_check.cpp does); the library exports the function as
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

}  // namespace genpc
