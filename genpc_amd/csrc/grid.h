// grid.h -- the uniform grid under every pruned search of the library (nn_grid.hip, emd_grid.hip, emd_auction.hip,
// nn_seeded.hip, knn_query.hip, knn.hip, icp.hip): the frame of a grid, the cell function, the sizing, the pieces of
// the LDS counting sort that the build kernels share, the bound by which a cell or a row of cells is skipped, and the walk over
// shells of cells of the k-nearest search.
//
// Bound.  cell(p) = clamp(floor(fl(fl(p - lo) * inv)), 0, G - 1) is monotone in p, and a point of
// cell c satisfies  lo + c h (1 - 3u) <= p < lo + (c + 1) h (1 + 3u)  (u = 2^-24, h = 1 / inv;
// border cells unbounded outwards).  With walls evaluated in fp32 and a slack of
// 16u (|lo| + G h + |q|) per axis, gap_a = max(0, wall_lo - s - q, q - wall_hi - s) <= |p_a - q_a|
// for every point p of the cell; the reference's distance is >= (sum gap_a^2)(1 - 6u); a cell is
// skipped iff  (sum gap_a^2)(1 - 2^-20) > best  (strictly: ties with lower indices are still
// found).  A search whose queries leave the box (icp.hip) gives the border cells the cloud's exact minimum and maximum for
// outer walls (grid_wall_gap takes any walls): every point satisfies mn <= p <= mx with no rounding at all, so the inequality
// holds a fortiori under the same slack.  Underflow only weakens the bound; an overflowing bound equals +inf and is only used
// against a finite best.  The helpers below ARE that arithmetic: a search that changes an intrinsic, an operand order or
// an association in its own copy has left the proof behind, which is why there are no copies -- but one: fps_grid.hip (gcell,
// box_margin, 0.9999f) keeps a grid and margins of its own that nothing here proves.  On these helpers it returns the same
// samples 0.8 - 2 % later, which is more than its own spread (DESIGN_NOTEBOOK.md, "icp_fused_kernel on grid.h; fps_grid.hip measured").
// The bound in reverse -- the cells that can hold a point within R of q -- is grid_cell_range below, for the same reason in one place.
// Tested by itself: csrc/probe.hip runs these helpers and grid.hip's builds on the inputs of tests/grid_cases.py (every fp32 wall and
// its neighbours, far queries, 2^-60 / 2^60, lattices, degenerate clouds), tests/test_gpu_grid.py checks each gap against |p - q| in
// exact arithmetic; the point that strays farthest outside its cell's fp32 walls uses 6 % of the slack (DESIGN_NOTEBOOK.md).
#pragma once
#include "common.h"
#include "ragged_table.h"

namespace genpc {

constexpr float kGridU16 = 9.5367431640625e-7f;      // 16 u
constexpr float kGridShrink = 0.99999905f;           // 1 - 2^-20

struct GridFrame {          // what the helpers need of a grid; the headers of the two cell numberings start with it
    float lo[3];
    float inv;              // cells per unit length (cubic cells of side h)
    float h;
    float slack[3];         // 16u (|lo| + (g + 1) h) per axis; grid_slack adds the query's 16u |q|
    int g[3];               // cells per axis
};

__device__ __forceinline__ int grid_cell1(float p, float lo, float inv, int g)
{
    const float t = __fmul_rn(__fsub_rn(p, lo), inv);
    int c = (int)floorf(t);          // NaN -> 0, +inf -> g - 1, -inf -> 0 on gfx950 (v_cvt_i32_f32 saturates; tests/test_gpu_grid.py); clouds with non-finite coordinates are searched without culling
    c = c < 0 ? 0 : c;
    return c > g - 1 ? g - 1 : c;
}

__device__ __forceinline__ float grid_slack(float slack, float q) { return slack + kGridU16 * fabsf(q); }

// lower bound of |p_a - q_a| over the points p with wl <= p_a <= wh (walls as fp32 values); s = grid_slack of q on that axis
__device__ __forceinline__ float grid_wall_gap(float wl, float wh, float q, float s)
{
    return fmaxf(0.0f, fmaxf((wl - s) - q, (q - s) - wh));
}

// lower bound of |p_a - q_a| over the points p of cells [c, c + w) of an axis (g cells of side h from lo; border cells
// unbounded outwards, or bounded by the cloud's exact minimum mn and maximum mx where the caller has them); s = grid_slack of q
// on that axis
__device__ __forceinline__ float grid_gap(int c, int w, int g, float lo, float h, float q, float s, float mn = -__builtin_inff(),
                                          float mx = __builtin_inff())
{
    const float wl = c > 0 ? __fadd_rn(lo, __fmul_rn((float)c, h)) : mn;
    const float wh = c + w < g ? __fadd_rn(lo, __fmul_rn((float)(c + w), h)) : mx;
    return grid_wall_gap(wl, wh, q, s);
}

// The Bound in reverse: the cells [c0, c1] of an axis that can hold a point p with |p_a - q_a| <= R (s = grid_slack of q on that
// axis).  cell() is monotone and (q - R) - s <= p <= (q + R) + s with room for the two roundings, so the cell of p lies between
// the cells of the two ends.  A NaN R gives [0, 0]: callers test R first.
struct GridRange { int c0, c1; };
__device__ __forceinline__ GridRange grid_cell_range(float q, float R, float s, float lo, float inv, int g)
{
    GridRange r;
    r.c0 = grid_cell1((q - R) - s, lo, inv, g);
    r.c1 = grid_cell1((q + R) + s, lo, inv, g);
    return r;
}
// the same range inside [b0, b1], the range of a wider radius: each end is clipped as soon as it is known
__device__ __forceinline__ GridRange grid_cell_range_in(float q, float R, float s, float lo, float inv, int g, int b0, int b1)
{
    GridRange r;
    r.c0 = max(b0, grid_cell1((q - R) - s, lo, inv, g));
    r.c1 = min(b1, grid_cell1((q + R) + s, lo, inv, g));
    return r;
}

// Block-wide box: every thread brings the (mn, mx) of its own points and leaves with the block's.  s_red: 6 floats per wave.
template <int BLOCK>
__device__ __forceinline__ void grid_block_box(float mn[3], float mx[3], float *s_red)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            mn[k] = fminf(mn[k], __shfl_xor(mn[k], o));
            mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) { s_red[wave * 6 + k] = mn[k]; s_red[wave * 6 + 3 + k] = mx[k]; }
    }
    __syncthreads();
    for (int w = 0; w < BLOCK / kWave; w++) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            mn[k] = fminf(mn[k], s_red[w * 6 + k]);
            mx[k] = fmaxf(mx[k], s_red[w * 6 + 3 + k]);
        }
    }
}

// The frame of g cells of side h from mn.  A side whose reciprocal is not a positive finite number: one cell of side 1.
__device__ __forceinline__ void grid_frame(const float mn[3], const int g[3], float h, GridFrame &F)
{
    float inv = 1.0f / h;
    const bool one = !(inv > 0.0f) || !(inv < __builtin_inff());
    if (one) { inv = 1.0f; h = 1.0f; }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int gk = one ? 1 : g[k];
        F.lo[k] = mn[k];
        F.g[k] = gk;
        F.slack[k] = kGridU16 * (fabsf(mn[k]) + (float)(gk + 1) * h);
    }
    F.inv = inv;
    F.h = h;
}

// Box (mn, mx) -> cubic cells of side h, about cells_target of them over the axes that are wider than h, at most
// cells_max as the numbering counts them: COARSE (nn_grid.hip: 4 x 4 x 4 blocks, partial ones padded) 64 x the product of
// (g + 3) / 4, else the product of g.  h grows by 1.26 (a doubling of the cell volume) up to REPS times to get there;
// a box that still does not fit becomes one cell of side 1.  An axis without a finite coordinate gets lo = 0.
template <int REPS, bool COARSE>
__device__ __forceinline__ void grid_size(float mn[3], float mx[3], int cells_target, int cells_max, GridFrame &F)
{
    float ext[3];
    bool act[3];
    int nact = 0;
    float emax = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (!(mn[k] <= mx[k])) { mn[k] = 0.0f; mx[k] = 0.0f; }      // no finite coordinate on this axis
        ext[k] = mx[k] - mn[k];
        if (!(ext[k] < __builtin_inff())) ext[k] = 0.0f;             // overflowing extent: one cell on this axis
        act[k] = ext[k] > 0.0f;
        nact += act[k] ? 1 : 0;
        emax = fmaxf(emax, ext[k]);
    }
    // (extents relative to the largest one: no overflow for clouds 1e-18 or 1e+18 across)
    float h = 0.0f;
    for (int it = 0; it < 3 && nact > 0; it++) {
        float vol = 1.0f;
        for (int k = 0; k < 3; k++) if (act[k]) vol *= ext[k] / emax;
        const float r = vol / (float)cells_target;
        h = emax * (nact == 3 ? cbrtf(r) : (nact == 2 ? sqrtf(r) : r));
        bool dropped = false;
        for (int k = 0; k < 3; k++) {
            if (act[k] && !(ext[k] > h)) { act[k] = false; nact--; dropped = true; }
        }
        if (!dropped) break;
    }
    if (!(h > 0.0f) || !(h < __builtin_inff()) || nact == 0) {
        h = 1.0f;
        for (int k = 0; k < 3; k++) act[k] = false;
    }
    int g[3];
    for (int rep = 0; rep < REPS; rep++) {
        long long cells = COARSE ? 64 : 1;
        for (int k = 0; k < 3; k++) {
            float q = act[k] ? ceilf(ext[k] / h) : 1.0f;
            if (!(q >= 1.0f)) q = 1.0f;
            if (q > 1024.0f) q = 1024.0f;
            g[k] = (int)q;
            cells *= COARSE ? (g[k] + 3) >> 2 : g[k];
        }
        if (cells <= cells_max) break;
        h *= 1.26f;
        if (rep == REPS - 1) { act[0] = act[1] = act[2] = false; h = 1.0f; }      // does not fit: one cell of side 1, as grid_frame's
    }
    for (int k = 0; k < 3; k++) if (!act[k]) g[k] = 1;
    grid_frame(mn, g, h, F);
}

// The scan between the histogram and the scatter of a counting sort in LDS: s_cnt[0 .. width) holds counts on entry and
// start offsets on return (a barrier passed either time); the first offset is the block's sum of `below`, each thread's
// count of the points in front of the slab.  Thread t owns [t per, (t + 1) per); per is odd (LDS banks).  s_w: 2 ints per wave.
template <int BLOCK>
__device__ __forceinline__ void grid_scan_counts(int *s_cnt, int width, int below, int *s_w)
{
    constexpr int kWaves = BLOCK / kWave;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int per = ((width + BLOCK - 1) / BLOCK) | 1;
    int sum = 0;
    for (int i = 0; i < per; i++) {
        const int q = threadIdx.x * per + i;
        if (q < width) { const int w = s_cnt[q]; s_cnt[q] = sum; sum += w; }
    }
    int inc = sum;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) below += __shfl_xor(below, o);
    if (lane == kWave - 1) s_w[wave] = inc;
    if (lane == 0) s_w[kWaves + wave] = below;
    __syncthreads();
    int base = inc - sum;
    for (int w = 0; w < kWaves; w++) {
        base += w < wave ? s_w[w] : 0;
        base += s_w[kWaves + w];
    }
    for (int i = 0; i < per; i++) {
        const int q = threadIdx.x * per + i;
        if (q < width) s_cnt[q] += base;
    }
    __syncthreads();
}

// ---- the x-fastest grid (grid.hip; emd_grid.hip, emd_auction.hip, nn_seeded.hip): cells numbered (cz g[1] + cy) g[0] + cx,
// so the cells [cx0, cx1] of a (cy, cz) ROW are one contiguous run of the sorted cloud ----
constexpr int kCellGridMaxCells = 15360;      // LDS counters of the build kernel (60 KiB)
struct CellGridHdr : GridFrame {     // one per batch element, written by cell_grid_build_kernel
    int cells;
    int bad;                // a non-finite coordinate or a negative / non-finite initial price: search without culling
};
// One cloud per batch element: hdr[b], start[b][cells_max + 1] (first sorted position of every cell), sorted[b][n] =
// (x, y, z, w).  price == null: w is the point's index.  price != null (the auction's objects): w is the price, or with
// price_sep the index while price_sep[b][position] gets the price; pos_of[b][point] = position and orig_of[b][position]
// = point when not null.
int launch_cell_grid_build(int b, int n, const float *xyz, const float *price, CellGridHdr *hdr, int *start, float4 *sorted, int *pos_of,
                           int *orig_of, int cells_target, int cells_max, hipStream_t st, float *price_sep = nullptr);

// The ragged sibling: cloud j is xyz[t.toff[j] .. t.toff[j + 1]), its grid sized for itself (ragged_cells_target / ragged_cells_max
// of ITS point count); hdr[j], its cell table at start + t.toff[j] + 65 j, sorted[t.toff[j] ..] = (x, y, z, index inside the
// cloud).  A cloud whose pair has no queries (t.qoff) is skipped and its pieces stay unwritten.  max_targets: the largest
// cloud that is built (sizes the LDS counters).  One launch for all clouds.
static_assert(kRaggedCellsCap == kCellGridMaxCells, "ragged_table.h restates the build's LDS budget");
int launch_cell_grid_build_ragged(const RaggedTable &t, int max_targets, const float *xyz, CellGridHdr *hdr, int *start, float4 *sorted,
                                  hipStream_t st);

// The walk of a k-nearest search (knn_query.hip, knn.hip) over a grid built by launch_cell_grid_build: ST = its start[].
// The lane walks shells of cells by Chebyshev distance r = 0, 1, 2 ... from the (clamped) cell of its query (qx, qy, qz).
// kth() is the caller's current k-th best distance, +inf while its list is short; run(p0, p1) visits the sorted positions
// [p0, p1).  A row, or a cell of an inner row, is skipped only if the Bound at the top is STRICTLY above kth() (ties with lower
// indices are still found); the walk stops once every cell outside the shells visited so far is that far, or at the grid's
// border.  While kth() is +inf nothing is above it.  The bounds are grid_gap / grid_slack / kGridShrink themselves.  A cloud
// with a non-finite coordinate (H.bad) is walked without culling: every cell is visited.
template <typename Kth, typename Run>
__device__ __forceinline__ void cell_grid_shell_walk(const CellGridHdr &H, const int *__restrict__ ST, float qx, float qy, float qz, Kth kth, Run run)
{
    const int gx = H.g[0], gy = H.g[1], gz = H.g[2];
    const float h = H.h;
    const bool cull = !H.bad;
    const float sx = grid_slack(H.slack[0], qx), sy = grid_slack(H.slack[1], qy), sz = grid_slack(H.slack[2], qz);
    const int cx = grid_cell1(qx, H.lo[0], H.inv, gx), cy = grid_cell1(qy, H.lo[1], H.inv, gy), cz = grid_cell1(qz, H.lo[2], H.inv, gz);
    const int rmax = max(max(max(cx, gx - 1 - cx), max(cy, gy - 1 - cy)), max(cz, gz - 1 - cz));
    for (int r = 0;; r++) {
        const int z0 = max(cz - r, 0), z1 = min(cz + r, gz - 1), y0 = max(cy - r, 0), y1 = min(cy + r, gy - 1);
        const int x0 = max(cx - r, 0), x1 = min(cx + r, gx - 1);
        for (int z = z0; z <= z1; z++) {
            const bool zface = z == cz - r || z == cz + r;
            const float gzv = grid_gap(z, 1, gz, H.lo[2], h, qz, sz);
            for (int y = y0; y <= y1; y++) {
                const float gyv = grid_gap(y, 1, gy, H.lo[1], h, qy, sy);
                const float lb0 = __fmaf_rn(gyv, gyv, __fmul_rn(gzv, gzv));
                if (cull && lb0 * kGridShrink > kth()) continue;          // strictly farther than the k-th best: not even a tie
                const int row = (z * gy + y) * gx;
                if (zface || y == cy - r || y == cy + r) {                 // a row of the shell's faces: one run
                    run(ST[row + x0], ST[row + x1 + 1]);
                } else {                                                   // an inner row: the shell's two cells (r > 0 here)
                    if (cx - r >= 0) {
                        const float gxv = grid_gap(cx - r, 1, gx, H.lo[0], h, qx, sx);
                        if (!(cull && __fmaf_rn(gxv, gxv, lb0) * kGridShrink > kth())) run(ST[row + cx - r], ST[row + cx - r + 1]);
                    }
                    if (cx + r < gx) {
                        const float gxv = grid_gap(cx + r, 1, gx, H.lo[0], h, qx, sx);
                        if (!(cull && __fmaf_rn(gxv, gxv, lb0) * kGridShrink > kth())) run(ST[row + cx + r], ST[row + cx + r + 1]);
                    }
                }
            }
        }
        if (r >= rmax) break;                // the whole grid has been visited
        if (cull) {
            // every cell not yet visited lies in one of the (at most six) slabs beyond the shell
            float m = __builtin_inff();
            if (cx - r > 0) m = fminf(m, grid_gap(0, cx - r, gx, H.lo[0], h, qx, sx));
            if (cx + r + 1 < gx) m = fminf(m, grid_gap(cx + r + 1, gx - (cx + r + 1), gx, H.lo[0], h, qx, sx));
            if (cy - r > 0) m = fminf(m, grid_gap(0, cy - r, gy, H.lo[1], h, qy, sy));
            if (cy + r + 1 < gy) m = fminf(m, grid_gap(cy + r + 1, gy - (cy + r + 1), gy, H.lo[1], h, qy, sy));
            if (cz - r > 0) m = fminf(m, grid_gap(0, cz - r, gz, H.lo[2], h, qz, sz));
            if (cz + r + 1 < gz) m = fminf(m, grid_gap(cz + r + 1, gz - (cz + r + 1), gz, H.lo[2], h, qz, sz));
            if (__fmul_rn(m, m) * kGridShrink > kth()) break;
        }
    }
}

}  // namespace genpc
