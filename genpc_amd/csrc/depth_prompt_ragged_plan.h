// depth_prompt_ragged_plan.h -- the limits, the work numbering, the launch count and the scratch of a genpc_depth_prompt_ragged
// call (depth_prompt_ragged.hip), decided from the host offset table and the image settings alone.  The entry point and its
// kernels read this header and decide nothing besides; the library exports it as genpc_depth_prompt_ragged_plan.
//
// Work numbering: scan j's points are cut into chunks of kDpChunk, one workgroup of kDpBlock threads each, thread t of chunk k
// owning the points k kDpChunk + kDpPer t .. + kDpPer - 1 of the scan.  Scan j's first chunk is item (off[j] >> 10) + j
// (ragged_offsets.h's numbering: the ranges do not overlap, a binary search of the table finds an item's scan, at most one
// item per scan finds nothing to do), (off[c] >> 10) + c items in all.
//
// THE SUMMATION ORDER of sums[j][r] (it depends on n_j alone, so a scan's sums are the same bits alone or anywhere in a batch):
//   1. a thread adds the (double) depths of its visible points in ascending index, starting from 0.0;
//   2. a wave adds its 64 threads' sums by the butterfly x += shuffle_xor(x, 32), 16, 8, 4, 2, 1;
//   3. a chunk's partial is ((w0 + w1) + w2) + w3 of its four waves;
//   4. lane l of the scan's one deciding wave adds the partials of chunks l, l + 64, ... in ascending order, starting from 0.0;
//   5. the 64 lanes' sums are added by the butterfly of step 2.
// No floating-point atomic anywhere; the boxes, the depth range and the pixel owners are integer atomic minima / maxima.
//
// Launches, whatever c is: ONE memset (box keys, depth-range keys and owner planes: all bytes 0xff) and kDpLaunches kernels:
//   box     (items x kDpBlock)   both cameras' exact NDC boxes, visible depth ranges and chunk partial sums
//   decide  (c x 64)             sums, chosen, status, the chosen camera's record (centre, extent, depth range)
//   write   (items x kDpBlock)   uv, depth, pix, visible of the chosen row; the owners of both stamps (atomicMax of the index)
//   image   (pixels x c)         the four images from the owner planes, flipped
// Host code only, no HIP: a plain C++ program can include it (tests/depth_prompt_ragged_plan_check.cpp does).
#pragma once
#include <stddef.h>
#include "ragged_offsets.h"

namespace genpc {

constexpr int kDpMaxScans = 256;                    // one table of 257 ints = 1028 bytes of the 4096 a kernel may take
constexpr int kDpMaxPoints = 1 << 28;               // all scans together
constexpr int kDpMaxRes = 4096;                     // image side
constexpr int kDpMaxStamp = 32;                     // point_size * mask_pixel_rate: a stamp of at most 63 x 63 pixels
constexpr long long kDpMaxOwnerInts = 1LL << 28;    // 2 c res^2: the owner planes stay within 1 GiB
constexpr int kDpBlock = 256;                       // threads of a workgroup
constexpr int kDpPer = 4;                           // points of a thread: three 16-byte loads of the packed coordinates
constexpr int kDpChunk = kDpBlock * kDpPer;         // points of a workgroup
constexpr int kDpChunkShift = 10;
static_assert(kDpChunk == 1 << kDpChunkShift, "the item numbering shifts by the chunk");
constexpr int kDpLaunches = 4;                      // kernels of a call
constexpr int kDpMemsets = 1;                       // memsets of a call
constexpr int kDpKeysPerScan = 2 * 4 + 2 * 2;       // per camera: four box keys; then per camera: two depth-range keys
constexpr int kDpRecFloats = 8;                     // per scan: cx, cy, sc, dmin, dmax, 3 spare

struct DepthPromptRaggedTable {
    int c;
    int off[kDpMaxScans + 1];
};

GENPC_RAGGED_HD inline int depth_prompt_items(int total, int c) { return (total >> kDpChunkShift) + c; }
GENPC_RAGGED_HD inline int depth_prompt_first_item(const int *off, int j) { return (off[j] >> kDpChunkShift) + j; }
GENPC_RAGGED_HD inline int depth_prompt_chunks(int n) { return (n + kDpChunk - 1) >> kDpChunkShift; }
// the scan an item belongs to
GENPC_RAGGED_HD inline int depth_prompt_scan_of(const DepthPromptRaggedTable &t, int item) { return ragged_item_owner(t.off, t.c, item, kDpChunkShift); }

struct DepthPromptRaggedPlan {
    int items;              // workgroups of the box and write launches
    int launches;           // kernels enqueued (0 when there is nothing to do)
    int memsets;
    int refused;            // scans without points: status -1, nothing of theirs written
    int first_refused;      // the lowest such scan, -1 when there is none
    long long fill_ints;    // 32-bit words the memset fills: keys, then owner planes
    long long ws_bytes;     // scratch of the call (ws_layout.h's rounding not counted)
};

// null when the call is taken, else what is wrong with it.  off may be null only when c == 0.
inline const char *depth_prompt_ragged_fault(int c, const int *off, int res, int point_size, int mask_pixel_rate)
{
    if (c < 0) return "negative number of scans";
    if (c > kDpMaxScans) return "more than 256 scans in one call";
    if (res < 1 || res > kDpMaxRes) return "res outside [1, 4096]";
    if (point_size < 1 || mask_pixel_rate < 1) return "point_size and mask_pixel_rate must be positive";
    if ((long long)point_size * mask_pixel_rate > kDpMaxStamp) return "point_size * mask_pixel_rate above 32";
    if (c == 0) return nullptr;
    if (!off) return "null offset table";
    if (const char *e = ragged_offsets_fault(c, off)) return e;
    if (off[c] > kDpMaxPoints) return "more than 2^28 points";
    if (2LL * c * res * res > kDpMaxOwnerInts) return "owner planes above 2^28 pixels (2 c res^2)";
    return nullptr;
}

// for a call depth_prompt_ragged_fault has taken
inline DepthPromptRaggedPlan depth_prompt_ragged_plan(int c, const int *off, int res)
{
    DepthPromptRaggedPlan p{0, 0, 0, 0, -1, 0, 0};
    if (c <= 0) return p;
    for (int j = 0; j < c; j++)
        if (off[j + 1] == off[j]) {
            if (p.first_refused < 0) p.first_refused = j;
            p.refused++;
        }
    p.items = depth_prompt_items(off[c], c);
    p.launches = kDpLaunches;
    p.memsets = kDpMemsets;
    p.fill_ints = (long long)c * kDpKeysPerScan + 2LL * c * res * res;
    p.ws_bytes = p.fill_ints * 4 + (long long)p.items * 2 * 8 + (long long)c * kDpRecFloats * 4;
    return p;
}

}  // namespace genpc
