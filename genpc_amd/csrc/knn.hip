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
#include "grid.h"
#include "../../include/genpc_hip.h"

namespace genpc {

constexpr int kKGBlock = 256;
template <int K, int FMA>
__global__ __launch_bounds__(kKGBlock) void knn_grid_kernel(int n, const float4 *__restrict__ S, const int *__restrict__ ST,
                                                            const CellGridHdr *__restrict__ hdr, float *__restrict__ mean_out)
{
    const int q = blockIdx.x * kKGBlock + threadIdx.x;
    if (q >= n) return;
    const CellGridHdr H = *hdr;
    const float4 me = S[q];
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
    mean_out[__float_as_int(me.w)] = (float)(acc / (double)cnt);
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
