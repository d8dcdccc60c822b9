// voxel_ragged.hip -- genpc_voxel_down_sample over a ragged batch: c clouds of any sizes, packed, each with its own voxel
// size, one call.  Cloud j's rows are the bits of genpc_voxel_down_sample on that cloud alone (voxel.hip): the grid is anchored
// at the cloud's OWN minimum minus half a voxel, the cell index is computed in double (voxel.h's voxel_point_key, the one
// statement of it), one output per occupied voxel in ascending (i, j, k), the mean in double over the voxel's points in
// ascending point index, colours the same way.
//
// The offsets and the voxel sizes ride BY VALUE in the kernel arguments (as ragged_table.h's pair table does): no copy is
// enqueued and nothing of the caller's host arrays is read after the entry point returns; 4 KiB of arguments bound c
// (kVoxelRaggedMaxClouds).  The launches, whatever c is:
//   voxel_ragged_bounds_kernel  six ordered-uint words per cloud (min, max), folded with integer atomics: order-independent.
//                               A workgroup owns one work item of ragged_items.h (1024 points of ONE cloud): it never straddles two.
//   voxel_ragged_key_kernel     per point: its key in its own cloud's grid, its packed index, its cloud's number; a bad
//                               coordinate raises its cloud's error word
//   rocprim radix sort x 2      the 63-bit key leaves no room for the cloud number, so (cloud, key, point) order comes from two
//                               STABLE passes: by key (64 bits), then by cloud number over only the bits c - 1 needs (none, and
//                               no pass, for c == 1).  The second pass reads its keys through the first pass's permutation.
//                               (rocprim::segmented_radix_sort is not used: its small-segment paths are not documented as
//                               stable, and the order of a voxel's points is the bits of its mean.)
//   voxel_ragged_head_kernel    a run head is a position where the key OR the cloud changes.  After the sort cloud j occupies the
//                               sorted positions [off[j], off[j + 1]): the cloud changes exactly at the off[j].
//   rocprim inclusive scan      ONE scan over all heads: rank
//   voxel_ragged_mean_kernel    the head of a run sums it in order, in double; its slot is off[j] + rank[i] - rank[off[j]]; the
//                               cloud's last position writes its count, rank[off[j + 1] - 1] - rank[off[j]] + 1.  No prefix over clouds.
//   voxel_ragged_fold_kernel    one thread per cloud: count 0 for an empty cloud, -1 for one whose error word is raised
#include "voxel.h"
#include "ragged_items.h"
#include "../../include/genpc_hip.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace genpc {

constexpr int kVoxelRaggedMaxClouds = GENPC_VOXEL_RAGGED_MAX_CLOUDS;
constexpr int kVoxelRaggedShift = 10;             // a work item of the bounds: 1024 points of one cloud, four a thread
static_assert(kVoxelRaggedMaxClouds <= kRaggedMaxPairs, "the bounds kernel deals its work through a RaggedTable");

struct VoxelRaggedArgs {
    int c;
    int off[kVoxelRaggedMaxClouds + 1];           // points of cloud j: [off[j], off[j + 1])
    double voxel[kVoxelRaggedMaxClouds];
    const float *xyz, *colors;                    // packed; colors may be null
    unsigned *bmin, *bmax;                        // [c, 3] each, ordered uints
    int *err;                                     // [c]
    unsigned long long *keys;                     // [total] by point
    unsigned *cloud;                              // [total] by point
    const int *order;                             // [total] point at each sorted position
    int *head, *rank;                             // [total] by sorted position
    float *out, *out_colors;
    int *out_counts;
};
static_assert(sizeof(VoxelRaggedArgs) <= 4096, "the table must fit the kernel arguments");

__global__ __launch_bounds__(kVBlock) void voxel_ragged_bounds_kernel(RaggedTable t, const float *__restrict__ xyz,
                                                                      unsigned *bmin, unsigned *bmax)
{
    __shared__ unsigned red[6][kVBlock / kWave];
    const int item = blockIdx.x;
    const int cloud = ragged_pair_of_shift(t, item, kVoxelRaggedShift);
    const int p0 = t.qoff[cloud], n = t.qoff[cloud + 1] - p0;
    const long long base = ragged_item_base_shift(t, cloud, item, kVoxelRaggedShift);
    if (base >= n) return;                                          // (uniform: the whole workgroup leaves)
    const int end = min(n, (int)base + (1 << kVoxelRaggedShift));
    unsigned mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
    for (int i = (int)base + threadIdx.x; i < end; i += kVBlock) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const unsigned o = f2ord(xyz[((size_t)p0 + i) * 3 + k]);
            mn[k] = o < mn[k] ? o : mn[k];
            mx[k] = o > mx[k] ? o : mx[k];
        }
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned a = (unsigned)__shfl_xor((int)mn[k], off, kWave), b = (unsigned)__shfl_xor((int)mx[k], off, kWave);
            mn[k] = a < mn[k] ? a : mn[k];
            mx[k] = b > mx[k] ? b : mx[k];
        }
        if (lane == 0) { red[k][wave] = mn[k]; red[3 + k][wave] = mx[k]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        unsigned v = red[threadIdx.x][0];
        for (int w = 1; w < kVBlock / kWave; w++) {
            const unsigned o = red[threadIdx.x][w];
            v = threadIdx.x < 3 ? (o < v ? o : v) : (o > v ? o : v);
        }
        if (threadIdx.x < 3) atomicMin(&bmin[cloud * 3 + threadIdx.x], v);
        else atomicMax(&bmax[cloud * 3 + threadIdx.x - 3], v);
    }
}

__global__ __launch_bounds__(kVBlock) void voxel_ragged_key_kernel(VoxelRaggedArgs a, int *__restrict__ idx)
{
    const int i = blockIdx.x * kVBlock + threadIdx.x;
    if (i >= a.off[a.c]) return;
    const int cloud = ragged_owner(a.off, a.c, i);          // (empty clouds are passed over)
    unsigned long long key;
    if (!voxel_point_key(a.xyz + (size_t)i * 3, a.voxel[cloud], a.bmin + cloud * 3, key)) a.err[cloud] = 1;
    a.keys[i] = key;
    a.cloud[i] = (unsigned)cloud;
    idx[i] = i;
}

// the second pass's key at a sorted position of the first: the cloud of the point that stands there
struct VoxelCloudOfPoint {
    const unsigned *cloud;
    __host__ __device__ unsigned operator()(int p) const { return cloud[p]; }
};

__global__ __launch_bounds__(kVBlock) void voxel_ragged_head_kernel(VoxelRaggedArgs a)
{
    const int i = blockIdx.x * kVBlock + threadIdx.x;
    if (i >= a.off[a.c]) return;
    const int cloud = ragged_owner(a.off, a.c, i);
    a.head[i] = (i == a.off[cloud] || a.keys[a.order[i]] != a.keys[a.order[i - 1]]) ? 1 : 0;
}

// rank[i] = inclusive scan of head over ALL clouds
__global__ __launch_bounds__(kVBlock) void voxel_ragged_mean_kernel(VoxelRaggedArgs a)
{
    const int i = blockIdx.x * kVBlock + threadIdx.x;
    if (i >= a.off[a.c]) return;
    const int cloud = ragged_owner(a.off, a.c, i);
    const int b = a.off[cloud], e = a.off[cloud + 1];
    const int first = a.rank[b];                           // (b is a head)
    if (i == e - 1) a.out_counts[cloud] = a.rank[i] - first + 1;
    if (!a.head[i]) return;
    double s[3] = {0.0, 0.0, 0.0}, c[3] = {0.0, 0.0, 0.0};
    int cnt = 0;
    for (int j = i; j < e && (j == i || !a.head[j]); j++) {
        const int p = a.order[j];
        s[0] += (double)a.xyz[(size_t)p * 3 + 0];
        s[1] += (double)a.xyz[(size_t)p * 3 + 1];
        s[2] += (double)a.xyz[(size_t)p * 3 + 2];
        if (a.colors) {
            c[0] += (double)a.colors[(size_t)p * 3 + 0];
            c[1] += (double)a.colors[(size_t)p * 3 + 1];
            c[2] += (double)a.colors[(size_t)p * 3 + 2];
        }
        cnt++;
    }
    const size_t slot = (size_t)b + (size_t)(a.rank[i] - first);
    float *o = a.out + slot * 3;
    o[0] = (float)(s[0] / cnt);
    o[1] = (float)(s[1] / cnt);
    o[2] = (float)(s[2] / cnt);
    if (a.colors && a.out_colors) {
        float *oc = a.out_colors + slot * 3;
        oc[0] = (float)(c[0] / cnt);
        oc[1] = (float)(c[1] / cnt);
        oc[2] = (float)(c[2] / cnt);
    }
}

__global__ __launch_bounds__(kVBlock) void voxel_ragged_fold_kernel(VoxelRaggedArgs a)
{
    const int j = blockIdx.x * kVBlock + threadIdx.x;
    if (j >= a.c) return;
    if (a.off[j + 1] == a.off[j]) a.out_counts[j] = 0;
    else if (a.err[j]) a.out_counts[j] = -1;
}

}  // namespace genpc

GENPC_API int genpc_voxel_down_sample_ragged(int c, const int *off, const float *xyz, const float *colors, const double *voxel_sizes,
                                             float *out, float *out_colors, int *out_counts, void *stream)
{
    using namespace genpc;
    const char *fn = "genpc_voxel_down_sample_ragged";
    // every refusal is decided here, before anything touches a device
    if (c < 0) return ragged_refuse(fn, "negative number of clouds");
    if (c == 0) return 1;
    if (c > kVoxelRaggedMaxClouds) return ragged_refuse(fn, "more than 256 clouds in one call");
    static_assert(kVoxelRaggedMaxClouds == 256, "the message above names the bound");
    if (!off || !voxel_sizes) return ragged_refuse(fn, "null offset or voxel size table");
    if (const char *fault = ragged_offsets_fault(c, off)) return ragged_refuse(fn, fault);
    if (off[c] > kRaggedMaxPoints) return ragged_refuse(fn, "more than 2^28 points");
    for (int j = 0; j < c; j++)
        if (!(voxel_sizes[j] > 0.0)) {
            char what[96];
            snprintf(what, sizeof what, "the voxel size of cloud %d is not > 0", j);
            return ragged_refuse(fn, what);
        }
    if (!out_counts || (off[c] > 0 && (!xyz || !out))) return ragged_refuse(fn, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int total = off[c];
    VoxelRaggedArgs a{};
    a.c = c;
    ragged_pad_copy(a.off, off, c);
    for (int j = 0; j < kVoxelRaggedMaxClouds; j++) a.voxel[j] = voxel_sizes[j < c ? j : c - 1];
    a.xyz = xyz; a.colors = colors; a.out = out; a.out_colors = out_colors; a.out_counts = out_counts;
    if (total == 0) {          // every cloud is empty: the counts alone
        if (!check(hipMemsetAsync(out_counts, 0, (size_t)c * sizeof(int), st), "hipMemsetAsync(voxel counts)")) return 0;
        return 1;
    }
    RaggedTable t;
    t.c = c;
    ragged_pad_copy(t.qoff, off, c);
    ragged_pad_copy(t.toff, off, c);
    unsigned cloud_bits = 0;
    while (cloud_bits < 32 && ((unsigned)(c - 1) >> cloud_bits) != 0) cloud_bits++;
    int *i0 = nullptr, *i1 = nullptr, *i2 = nullptr;
    unsigned long long *k1 = nullptr;
    unsigned *c2 = nullptr, *hdr = nullptr;
    char *tmp = nullptr;
    const VoxelCloudOfPoint cloud_of{nullptr};
    size_t sort_bytes = 0, sort2_bytes = 0, scan_bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, sort_bytes, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                    (const int *)nullptr, (int *)nullptr, (size_t)total, 0u, 63u, st);
    if (cloud_bits)
        (void)rocprim::radix_sort_pairs(nullptr, sort2_bytes, rocprim::make_transform_iterator((const int *)nullptr, cloud_of), (unsigned *)nullptr,
                                        (const int *)nullptr, (int *)nullptr, (size_t)total, 0u, cloud_bits, st);
    (void)rocprim::inclusive_scan(nullptr, scan_bytes, (const int *)nullptr, (int *)nullptr, (size_t)total, rocprim::plus<int>(), st);
    size_t tmp_bytes = sort_bytes > sort2_bytes ? sort_bytes : sort2_bytes;
    tmp_bytes = WsLayout::up(tmp_bytes > scan_bytes ? tmp_bytes : scan_bytes);
    WsLayout L;
    L.add(hdr, (size_t)7 * c);          // min [c,3] | max [c,3] | error words [c]
    L.add(a.keys, total);
    L.add(k1, total);
    L.add(a.cloud, total);
    L.add_if(cloud_bits != 0, c2, total);
    L.add(i0, total);
    L.add(i1, total);
    L.add_if(cloud_bits != 0, i2, total);
    L.add(a.head, total);
    L.add(a.rank, total);
    L.add(tmp, tmp_bytes);
    if (!ws_alloc(L, kWsVoxelRagged, st)) return 0;
    a.bmin = hdr; a.bmax = hdr + 3 * c; a.err = (int *)(hdr + 6 * c);
    a.order = cloud_bits ? i2 : i1;
    // min = 0xffffffff, max = 0, error words = 0
    if (!check(hipMemsetAsync(a.bmin, 0xff, (size_t)3 * c * sizeof(unsigned), st), "hipMemsetAsync(voxel bounds)")) return 0;
    if (!check(hipMemsetAsync(a.bmax, 0, (size_t)4 * c * sizeof(unsigned), st), "hipMemsetAsync(voxel bounds)")) return 0;
    const int grid = ceil_div(total, kVBlock);
    const int items = (int)ragged_items_shift(total, c, kVoxelRaggedShift);
    hipLaunchKernelGGL(voxel_ragged_bounds_kernel, dim3(items), dim3(kVBlock), 0, st, t, xyz, a.bmin, a.bmax);
    hipLaunchKernelGGL(voxel_ragged_key_kernel, dim3(grid), dim3(kVBlock), 0, st, a, i0);
    if (!check(hipGetLastError(), "voxel_down_sample_ragged launch")) return 0;
    size_t sb = tmp_bytes;
    if (!check(rocprim::radix_sort_pairs(tmp, sb, (const unsigned long long *)a.keys, k1, (const int *)i0, i1, (size_t)total, 0u, 63u, st),
               "voxel radix sort (keys)"))
        return 0;
    if (cloud_bits) {
        sb = tmp_bytes;
        const VoxelCloudOfPoint by_cloud{a.cloud};
        if (!check(rocprim::radix_sort_pairs(tmp, sb, rocprim::make_transform_iterator((const int *)i1, by_cloud), c2, (const int *)i1, i2,
                                             (size_t)total, 0u, cloud_bits, st),
                   "voxel radix sort (clouds)"))
            return 0;
    }
    hipLaunchKernelGGL(voxel_ragged_head_kernel, dim3(grid), dim3(kVBlock), 0, st, a);
    sb = tmp_bytes;
    if (!check(rocprim::inclusive_scan(tmp, sb, (const int *)a.head, a.rank, (size_t)total, rocprim::plus<int>(), st), "voxel scan")) return 0;
    hipLaunchKernelGGL(voxel_ragged_mean_kernel, dim3(grid), dim3(kVBlock), 0, st, a);
    hipLaunchKernelGGL(voxel_ragged_fold_kernel, dim3(ceil_div(c, kVBlock)), dim3(kVBlock), 0, st, a);
    return check(hipGetLastError(), "voxel_down_sample_ragged launch") ? 1 : 0;
}
