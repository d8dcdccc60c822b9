// knn.hip -- mean distance to the k nearest neighbours within one cloud, the
// quantity behind open3d's remove_statistical_outlier, which closes the fusion tail
// of reg() (reg_xyz.py:217 -> utils/dataUtils.py:648-662).
// open3d is absent and unpinned; its published algorithm is restated: for every
// point the k nearest points of the SAME cloud (the point itself included, at
// distance 0), mean of their Euclidean distances; a point survives when its mean is
// below cloud_mean + std_ratio * cloud_std (sample standard deviation).
//
// The cloud is sorted once per call into the x-fastest grid of grid.h (launch_cell_grid_build); the queries are the sorted
// points themselves, one lane per sorted position, so a wave's lanes are neighbours.  The k best squared distances
// (sqdist<FMA> of common.h in the call's arithmetic mode) live in registers as an ascending list; the insertion is one v_med3
// per list slot:  t'[i] = med3(d, t[i-1], t[i]).  The lane visits the targets by grid.h's cell_grid_shell_walk, which skips
// and stops against the k-th best.  Equal distances at the k-th place carry equal values, so the mean does not depend on
// which of them is kept: bit-exact with the oracle (sum of square roots in ascending order, in double).  NaN and infinite
// distances never enter a list; a cloud with a non-finite coordinate (CellGridHdr.bad) is walked without culling, a point with
// one gets 0 / 0 = NaN, every other point the mean it has without those points.
// One path for every size: a tiny or degenerate cloud is a one-cell grid.
//
// The ragged forms (genpc_knn_mean_distance_ragged, genpc_outlier_filter_ragged): c clouds of any sizes, packed, one call.
//   * grid.hip's ragged build sorts every cloud into a grid of its own (ragged_table.h, qoff == toff: a cloud is its own
//     queries).  Its cells are coarser than launch_knn's; the search is exact on any grid, so the means are the same bits.
//   * knn_ragged_kernel: the same search (knn_mean_of, one body for both kernels).  A workgroup serves up to 256 sorted
//     positions of ONE cloud: blockIdx.x is a work item of ragged_items.h's numbering with shift 8, the cloud comes from a
//     binary search of the table in the kernel arguments (uniform: scalar loads).
//   * outlier_stats_kernel (the filter only): one workgroup of 1024 per cloud makes mean, std and threshold in the summation
//     order include/genpc_hip.h defines -- partial p[t] of thread t, then a halving tree in LDS, every operation rounded on
//     its own -- and then the mask and its count.  The order is a function of the cloud's size alone.
#include "grid.h"
#include "ragged_items.h"
#include "../../include/genpc_hip.h"

namespace genpc {

constexpr int kKGBlock = 256;
// THE search of one sorted position (knn_grid_kernel, knn_ragged_kernel): the cloud's grid (H, its cell table ST, its sorted
// points S) and the lane's own point `me`; returns the mean of the listed distances.
template <int K, int FMA>
__device__ __forceinline__ float knn_mean_of(const CellGridHdr &H, const float4 *__restrict__ S, const int *__restrict__ ST, const float4 me)
{
    float t[K];
#pragma unroll
    for (int i = 0; i < K; i++) t[i] = __builtin_inff();
    auto kth = [&]() { return t[K - 1]; };          // +inf while fewer than K are listed
    auto run = [&](int p0, int p1) {                // the targets at positions [p0, p1) of the sorted cloud
        for (int p = p0; p < p1; p++) {
            const float4 v = S[p];
            const float d = sqdist<FMA>(v.x - me.x, v.y - me.y, v.z - me.z);
            if (d < t[K - 1]) {
                // sorted insertion, the largest falls off
#pragma unroll
                for (int i = K - 1; i > 0; i--) t[i] = __builtin_amdgcn_fmed3f(d, t[i - 1], t[i]);
                t[0] = fminf(d, t[0]);
            }
        }
    };
    cell_grid_shell_walk(H, ST, me.x, me.y, me.z, kth, run);
    double acc = 0.0;
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < K; i++) {
        if (t[i] < __builtin_inff()) {           // fewer than K points in the cloud
            acc += sqrt((double)t[i]);
            cnt++;
        }
    }
    return (float)(acc / (double)cnt);
}

template <int K, int FMA>
__global__ __launch_bounds__(kKGBlock) void knn_grid_kernel(int n, const float4 *__restrict__ S, const int *__restrict__ ST,
                                                            const CellGridHdr *__restrict__ hdr, float *__restrict__ mean_out)
{
    const int q = blockIdx.x * kKGBlock + threadIdx.x;
    if (q >= n) return;
    const CellGridHdr H = *hdr;
    const float4 me = S[q];
    mean_out[__float_as_int(me.w)] = knn_mean_of<K, FMA>(H, S, ST, me);
}

template <int K>
static int launch_knn(int n, const float *xyz, float *out, hipStream_t st)
{
    CellGridHdr *hdr; int *start; float4 *sorted;
    WsLayout L;
    L.add(hdr, 1);
    L.add(start, (size_t)kCellGridMaxCells + 1);
    L.add(sorted, n);
    if (!ws_alloc(L, kWsKnnMean, st)) return 0;
    // cells of about half a point: the shells around a query stay small while its list fills
    int target = 2 * n;
    target = target < 64 ? 64 : (target > 8192 ? 8192 : target);
    if (!launch_cell_grid_build(1, n, xyz, nullptr, hdr, start, sorted, nullptr, nullptr, target, kCellGridMaxCells, st)) return 0;
    const int blocks = ceil_div(n, kKGBlock);
    if (arith_mode() != 0)
        hipLaunchKernelGGL((knn_grid_kernel<K, 1>), dim3(blocks), dim3(kKGBlock), 0, st, n, (const float4 *)sorted, (const int *)start, (const CellGridHdr *)hdr, out);
    else
        hipLaunchKernelGGL((knn_grid_kernel<K, 0>), dim3(blocks), dim3(kKGBlock), 0, st, n, (const float4 *)sorted, (const int *)start, (const CellGridHdr *)hdr, out);
    return check(hipGetLastError(), "knn_grid_kernel launch") ? 1 : 0;
}

constexpr int kKRShift = 8;                       // a work item: kKGBlock sorted positions of one cloud
static_assert((1 << kKRShift) == kKGBlock, "a work item is what a workgroup of the search owns");
constexpr int kOSBlock = 1024;                    // the partial sums of S(v): include/genpc_hip.h fixes the number

struct KnnRaggedArgs {
    RaggedTable t;                 // qoff == toff: the clouds
    const float4 *sorted;          // packed, every cloud's slice in its own cell order: (x, y, z, index inside the cloud)
    const int *start;              // cloud j's cell table at off[j] + 65 j
    const CellGridHdr *hdr;        // [c]
    float *mean;                   // packed like the clouds
    double std_ratio;
    double *stats;                 // [c, 3] or null
    unsigned char *keep;           // packed like the clouds
    int *kept;                     // [c] or null
};
static_assert(sizeof(KnnRaggedArgs) <= 4096, "the cloud table must fit the kernel arguments");

template <int K, int FMA>
__global__ __launch_bounds__(kKGBlock) void knn_ragged_kernel(KnnRaggedArgs a)
{
    const int item = blockIdx.x;
    const int cloud = ragged_pair_of_shift(a.t, item, kKRShift);
    const int p0 = a.t.qoff[cloud], n = a.t.qoff[cloud + 1] - p0;
    const long long q = ragged_item_base_shift(a.t, cloud, item, kKRShift) + threadIdx.x;
    if (q >= n) return;
    const CellGridHdr H = a.hdr[cloud];
    const float4 *__restrict__ S = a.sorted + p0;
    const int *__restrict__ ST = a.start + ((size_t)p0 + (size_t)kRaggedStartPad * cloud);
    const float4 me = S[q];
    a.mean[(size_t)p0 + __float_as_int(me.w)] = knn_mean_of<K, FMA>(H, S, ST, me);
}

// S(v) of include/genpc_hip.h from the threads' partials: the halving tree.  Every thread gets p[0].
__device__ __forceinline__ double outlier_tree_sum(double p, double *s_p)
{
    __syncthreads();                              // (the previous sum's p[0] has been read by all)
    s_p[threadIdx.x] = p;
    __syncthreads();
    for (int w = kOSBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s_p[threadIdx.x] = __dadd_rn(s_p[threadIdx.x], s_p[threadIdx.x + w]);
        __syncthreads();
    }
    return s_p[0];
}

__global__ __launch_bounds__(kOSBlock) void outlier_stats_kernel(KnnRaggedArgs a)
{
    __shared__ double s_p[kOSBlock];
    __shared__ int s_n[kOSBlock / kWave];
    const int cloud = blockIdx.x;
    const int p0 = a.t.qoff[cloud], n = a.t.qoff[cloud + 1] - p0;
    if (n == 0) {                                 // (uniform: the whole workgroup leaves)
        if (threadIdx.x == 0) {
            const double nan = __builtin_nan("");
            if (a.stats) { a.stats[cloud * 3 + 0] = nan; a.stats[cloud * 3 + 1] = nan; a.stats[cloud * 3 + 2] = nan; }
            if (a.kept) a.kept[cloud] = 0;
        }
        return;
    }
    const float *__restrict__ M = a.mean + p0;
    // (unrolled: four loads are in flight at once; the additions keep their order)
    double p = 0.0;
#pragma unroll 4
    for (int i = threadIdx.x; i < n; i += kOSBlock) p = __dadd_rn(p, (double)M[i]);
    const double mean = __ddiv_rn(outlier_tree_sum(p, s_p), (double)n);
    p = 0.0;
#pragma unroll 4
    for (int i = threadIdx.x; i < n; i += kOSBlock) {
        const double d = __dsub_rn((double)M[i], mean);
        p = __dadd_rn(p, __dmul_rn(d, d));
    }
    const double sd = __dsqrt_rn(__ddiv_rn(outlier_tree_sum(p, s_p), (double)(n - 1)));
    const double thr = __dadd_rn(mean, __dmul_rn(a.std_ratio, sd));
    unsigned char *__restrict__ keep = a.keep + p0;
    int ones = 0;
#pragma unroll 4
    for (int i = threadIdx.x; i < n; i += kOSBlock) {
        const int k = (double)M[i] < thr ? 1 : 0;
        keep[i] = (unsigned char)k;
        ones += k;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) ones += __shfl_xor(ones, o);
    if ((threadIdx.x & (kWave - 1)) == 0) s_n[threadIdx.x / kWave] = ones;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < kOSBlock / kWave; w++) total += s_n[w];
        if (a.kept) a.kept[cloud] = total;
        if (a.stats) { a.stats[cloud * 3 + 0] = mean; a.stats[cloud * 3 + 1] = sd; a.stats[cloud * 3 + 2] = thr; }
    }
}

template <int K>
static int launch_knn_ragged(const KnnRaggedArgs &a, hipStream_t st)
{
    const unsigned grid = (unsigned)ragged_items_shift(a.t.qoff[a.t.c], a.t.c, kKRShift);
    if (arith_mode() != 0) hipLaunchKernelGGL((knn_ragged_kernel<K, 1>), dim3(grid), dim3(kKGBlock), 0, st, a);
    else hipLaunchKernelGGL((knn_ragged_kernel<K, 0>), dim3(grid), dim3(kKGBlock), 0, st, a);
    return check(hipGetLastError(), "knn_ragged_kernel launch") ? 1 : 0;
}

// Both ragged entry points: `filter` false stops after the search (mean_out is the result), true goes on to the statistics.
static int knn_ragged(const char *who, int c, const int *off, const float *xyz, int k, bool filter, double std_ratio, float *mean_out,
                      double *stats, unsigned char *keep, int *kept, hipStream_t st)
{
    KnnRaggedArgs a{};
    int max_points = 0;
    const char *err = nullptr;
    const int rc = ragged_table_fill(c, off, off, a.t, &max_points, &err);
    if (rc < 0) return ragged_refuse(who, err);
    if (k != 8 && k != 16 && k != 20 && k != 32) return ragged_refuse(who, "k must be 8, 16, 20 or 32");
    if (rc == 0) return 1;
    if (!xyz || (filter ? !keep : !mean_out)) return ragged_refuse(who, "null pointer");
    const int total = a.t.qoff[c];
    a.std_ratio = std_ratio; a.stats = stats; a.keep = keep; a.kept = kept; a.mean = mean_out;
    WsLayout L;
    L.add(a.hdr, c);
    L.add(a.start, (size_t)ragged_start_len(total, c));
    L.add(a.sorted, (size_t)total);
    float *ws_mean = nullptr;
    L.add_if(!mean_out, ws_mean, (size_t)total);
    if (!ws_alloc(L, kWsKnnMeanRagged, st)) return 0;
    if (!mean_out) a.mean = ws_mean;
    if (!launch_cell_grid_build_ragged(a.t, max_points, xyz, (CellGridHdr *)a.hdr, (int *)a.start, (float4 *)a.sorted, st)) return 0;
    int ok;
    switch (k) {
    case 8: ok = launch_knn_ragged<8>(a, st); break;
    case 16: ok = launch_knn_ragged<16>(a, st); break;
    case 20: ok = launch_knn_ragged<20>(a, st); break;
    default: ok = launch_knn_ragged<32>(a, st); break;
    }
    if (!ok || !filter) return ok;
    hipLaunchKernelGGL(outlier_stats_kernel, dim3(c), dim3(kOSBlock), 0, st, a);
    return check(hipGetLastError(), "outlier_stats_kernel launch") ? 1 : 0;
}

}  // namespace genpc

GENPC_API int genpc_knn_mean_distance(int n, const float *xyz, int k, float *mean_out, void *stream)
{
    using namespace genpc;
    if (n <= 0) return 1;
    hipStream_t st = (hipStream_t)stream;
    switch (k) {
    case 8: return launch_knn<8>(n, xyz, mean_out, st);
    case 16: return launch_knn<16>(n, xyz, mean_out, st);
    case 20: return launch_knn<20>(n, xyz, mean_out, st);
    case 32: return launch_knn<32>(n, xyz, mean_out, st);
    default:
        fprintf(stderr, "genpc_knn_mean_distance: k must be 8, 16, 20 or 32\n");
        return -1;
    }
}

GENPC_API int genpc_knn_mean_distance_ragged(int c, const int *off, const float *xyz, int k, float *mean_out, void *stream)
{
    return genpc::knn_ragged("genpc_knn_mean_distance_ragged", c, off, xyz, k, false, 0.0, mean_out, nullptr, nullptr, nullptr,
                             (hipStream_t)stream);
}

GENPC_API int genpc_outlier_filter_ragged(int c, const int *off, const float *xyz, int k, double std_ratio, float *mean_out, double *stats,
                                          unsigned char *keep, int *kept, void *stream)
{
    return genpc::knn_ragged("genpc_outlier_filter_ragged", c, off, xyz, k, true, std_ratio, mean_out, stats, keep, kept, (hipStream_t)stream);
}
