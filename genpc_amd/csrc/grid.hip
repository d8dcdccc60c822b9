// grid.hip -- builds the x-fastest grid of grid.h: one cloud per batch element sorted to cell order, once per call.
#include "grid.h"

namespace genpc {

constexpr int kCGBlock = 1024;          // build kernel: K blocks per cloud
constexpr int kCGWaves = kCGBlock / kWave;

// Exact bounding box of the cloud, grid_size, counting sort in LDS; outputs as grid.h describes them.  The order inside a
// cell is whatever the LDS atomics give: it does not reach any result.
__global__ __launch_bounds__(kCGBlock) void cell_grid_build_kernel(int n, const float *__restrict__ xyz, const float *__restrict__ price,
                                                                   CellGridHdr *__restrict__ hdr, int *__restrict__ start,
                                                                   float4 *__restrict__ sorted, int *__restrict__ pos_of,
                                                                   int *__restrict__ orig_of, int cells_target, int cells_max, int K,
                                                                   float *__restrict__ price_sep)
{
    // K blocks per cloud (a single cloud on one CU took 48 us of a 1 ms call): block k sorts the cells [c0, c1) of the
    // cell index space -- a contiguous piece of the sorted output.  Every block reads ALL points of the cloud (box, cell of
    // each point: arithmetic only), but only the points of its own cells go through the LDS histogram, the scan and the
    // scatter; the piece's first output position is the number of points in lower cells, which the block counts while it
    // classifies: no communication between the blocks (as nn_grid.hip's grid_build_kernel does with coarse rows).
    extern __shared__ int s_cnt[];            // cells_max counters, then 2 kCGWaves ints, then 6 kCGWaves floats
    int *s_w = s_cnt + cells_max;
    float *s_red = (float *)(s_w + 2 * kCGWaves);
    const int batch = blockIdx.x / K, kb = blockIdx.x % K;
    const float *__restrict__ P = xyz + (size_t)batch * n * 3;
    float mn[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float mx[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    int bad = 0;
    const float *__restrict__ PR0 = price ? price + (size_t)batch * n : nullptr;
    for (int j = threadIdx.x; j < n; j += kCGBlock) {
        if (PR0) bad |= !(PR0[j] >= 0.0f && PR0[j] < __builtin_inff());      // the auction's culling needs prices >= 0 (the caller's initial state: zeros)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float w = P[(size_t)j * 3 + k];
            if (fabsf(w) < __builtin_inff()) {
                mn[k] = fminf(mn[k], w);
                mx[k] = fmaxf(mx[k], w);
            } else {
                bad = 1;
            }
        }
    }
    grid_block_box<kCGBlock>(mn, mx, s_red);
    bad = __syncthreads_or(bad);
    CellGridHdr H;
    grid_size<16, false>(mn, mx, cells_target, cells_max, H);
    H.cells = H.g[0] * H.g[1] * H.g[2];
    H.bad = bad;
    if (threadIdx.x == 0 && kb == 0) hdr[batch] = H;
    const int cells = H.cells;
    const int c0 = (int)(((long long)kb * cells) / K), c1 = (int)(((long long)(kb + 1) * cells) / K), width = c1 - c0;
    for (int i = threadIdx.x; i < width; i += kCGBlock) s_cnt[i] = 0;
    __syncthreads();
    auto cell_of = [&](int j) {
        const int cx = grid_cell1(P[(size_t)j * 3 + 0], H.lo[0], H.inv, H.g[0]), cy = grid_cell1(P[(size_t)j * 3 + 1], H.lo[1], H.inv, H.g[1]);
        const int cz = grid_cell1(P[(size_t)j * 3 + 2], H.lo[2], H.inv, H.g[2]);
        return (cz * H.g[1] + cy) * H.g[0] + cx;
    };
    int below = 0;
    for (int j = threadIdx.x; j < n; j += kCGBlock) {
        const int c = cell_of(j);
        below += c < c0 ? 1 : 0;
        if (c >= c0 && c < c1) atomicAdd(&s_cnt[c - c0], 1);
    }
    __syncthreads();
    grid_scan_counts<kCGBlock>(s_cnt, width, below, s_w);
    int *st = start + (size_t)batch * (cells_max + 1);
    for (int i = threadIdx.x; i < width; i += kCGBlock) st[c0 + i] = s_cnt[i];
    if (threadIdx.x == 0 && kb == K - 1) st[cells] = n;
    __syncthreads();
    float4 *out = sorted + (size_t)batch * n;
    int *po = pos_of ? pos_of + (size_t)batch * n : nullptr;
    int *ps = orig_of ? orig_of + (size_t)batch * n : nullptr;
    for (int j = threadIdx.x; j < n; j += kCGBlock) {
        const int c = cell_of(j);
        if (c < c0 || c >= c1) continue;
        const int pos = atomicAdd(&s_cnt[c - c0], 1);
        out[pos] = make_float4(P[(size_t)j * 3 + 0], P[(size_t)j * 3 + 1], P[(size_t)j * 3 + 2], (PR0 && !price_sep) ? PR0[j] : __int_as_float(j));
        if (price_sep) price_sep[(size_t)batch * n + pos] = PR0 ? PR0[j] : 0.0f;
        if (po) po[j] = pos;
        if (ps) ps[pos] = j;
    }
}

int launch_cell_grid_build(int b, int n, const float *xyz, const float *price, CellGridHdr *hdr, int *start, float4 *sorted, int *pos_of,
                           int *orig_of, int cells_target, int cells_max, hipStream_t st, float *price_sep)
{
    const size_t lds = ((size_t)cells_max + (2 + 6) * kCGWaves) * sizeof(int);
    // pieces per cloud: enough blocks to spread a few clouds over the chip, one when there are many clouds anyway
    const int K = b >= 32 ? 1 : (b >= 8 ? 2 : (n >= 8192 ? 8 : 4));
    hipLaunchKernelGGL(cell_grid_build_kernel, dim3(b * K), dim3(kCGBlock), lds, st, n, xyz, price, hdr, start, sorted, pos_of, orig_of,
                       cells_target, cells_max, K, price_sep);
    return check(hipGetLastError(), "cell_grid_build_kernel launch") ? 1 : 0;
}

// The same build for clouds of different sizes (grid.h, ragged_table.h): block (cloud, piece) reads its cloud's slice and its own
// grid budget from the table in the kernel arguments; everything else is cell_grid_build_kernel's, without the prices.
__global__ __launch_bounds__(kCGBlock) void cell_grid_build_ragged_kernel(RaggedTable t, const float *__restrict__ xyz,
                                                                          CellGridHdr *__restrict__ hdr, int *__restrict__ start,
                                                                          float4 *__restrict__ sorted, int lds_cells, int K)
{
    extern __shared__ int s_cnt[];            // lds_cells counters, then 2 kCGWaves ints, then 6 kCGWaves floats
    int *s_w = s_cnt + lds_cells;
    float *s_red = (float *)(s_w + 2 * kCGWaves);
    const int cloud = blockIdx.x / K, kb = blockIdx.x % K;
    if (t.qoff[cloud + 1] == t.qoff[cloud]) return;          // nobody asks (the whole block leaves: no barrier is left waiting)
    const int p0 = t.toff[cloud], n = t.toff[cloud + 1] - p0;
    const float *__restrict__ P = xyz + (size_t)p0 * 3;
    float mn[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float mx[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    int bad = 0;
    for (int j = threadIdx.x; j < n; j += kCGBlock) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float w = P[(size_t)j * 3 + k];
            if (fabsf(w) < __builtin_inff()) {
                mn[k] = fminf(mn[k], w);
                mx[k] = fmaxf(mx[k], w);
            } else {
                bad = 1;
            }
        }
    }
    grid_block_box<kCGBlock>(mn, mx, s_red);
    bad = __syncthreads_or(bad);
    CellGridHdr H;
    grid_size<16, false>(mn, mx, ragged_cells_target(n), ragged_cells_max(n), H);
    H.cells = H.g[0] * H.g[1] * H.g[2];
    H.bad = bad;
    if (threadIdx.x == 0 && kb == 0) hdr[cloud] = H;
    const int cells = H.cells;
    const int c0 = (int)(((long long)kb * cells) / K), c1 = (int)(((long long)(kb + 1) * cells) / K), width = c1 - c0;
    for (int i = threadIdx.x; i < width; i += kCGBlock) s_cnt[i] = 0;
    __syncthreads();
    auto cell_of = [&](int j) {
        const int cx = grid_cell1(P[(size_t)j * 3 + 0], H.lo[0], H.inv, H.g[0]), cy = grid_cell1(P[(size_t)j * 3 + 1], H.lo[1], H.inv, H.g[1]);
        const int cz = grid_cell1(P[(size_t)j * 3 + 2], H.lo[2], H.inv, H.g[2]);
        return (cz * H.g[1] + cy) * H.g[0] + cx;
    };
    int below = 0;
    for (int j = threadIdx.x; j < n; j += kCGBlock) {
        const int c = cell_of(j);
        below += c < c0 ? 1 : 0;
        if (c >= c0 && c < c1) atomicAdd(&s_cnt[c - c0], 1);
    }
    __syncthreads();
    grid_scan_counts<kCGBlock>(s_cnt, width, below, s_w);
    int *st = start + ((size_t)p0 + (size_t)kRaggedStartPad * cloud);
    for (int i = threadIdx.x; i < width; i += kCGBlock) st[c0 + i] = s_cnt[i];
    if (threadIdx.x == 0 && kb == K - 1) st[cells] = n;
    __syncthreads();
    float4 *out = sorted + p0;
    for (int j = threadIdx.x; j < n; j += kCGBlock) {
        const int c = cell_of(j);
        if (c < c0 || c >= c1) continue;
        const int pos = atomicAdd(&s_cnt[c - c0], 1);
        out[pos] = make_float4(P[(size_t)j * 3 + 0], P[(size_t)j * 3 + 1], P[(size_t)j * 3 + 2], __int_as_float(j));
    }
}

int launch_cell_grid_build_ragged(const RaggedTable &t, int max_targets, const float *xyz, CellGridHdr *hdr, int *start, float4 *sorted,
                                  hipStream_t st)
{
    const int lds_cells = ragged_cells_max(max_targets);
    const size_t lds = ((size_t)lds_cells + (2 + 6) * kCGWaves) * sizeof(int);
    // pieces per cloud, as above: a few clouds are spread over the chip, many fill it anyway
    const int K = t.c >= 32 ? 1 : (t.c >= 8 ? 2 : 4);
    hipLaunchKernelGGL(cell_grid_build_ragged_kernel, dim3(t.c * K), dim3(kCGBlock), lds, st, t, xyz, hdr, start, sorted, lds_cells, K);
    return check(hipGetLastError(), "cell_grid_build_ragged_kernel launch") ? 1 : 0;
}

}  // namespace genpc
