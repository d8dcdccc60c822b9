// uhd.hip -- the directed (unidirectional) Hausdorff distance from queries [B, N, 3] to targets [B, M, 3], exact in fp64.
//
// The reference's UHD (metric.py:105-132) is max_i min_j of scipy's cdist(partial, complete, 'euclidean'): float64,
// d = u[k] - v[k], s = ((dx*dx) + (dy*dy)) + (dz*dz), sqrt(s), no fused multiply-add.  sqrt is monotone, so the answer is
// sqrt(max_i min_j s_ij) and the root is left to the caller; here every pair's s is evaluated in exactly that order on
// the fp32 inputs widened to fp64 (the library is built with -ffp-contract=off: nothing re-fuses it).
//   * uhd_pairs_kernel: all pairs.  A workgroup stages one tile of kUhdTile targets in LDS as doubles; a lane owns
//     kUhdQ queries in registers and walks the tile (every lane reads the same LDS address: a broadcast), 9 fp64
//     operations a pair, the minimum kept with fmin -- no index in the hot loop.  The target range is split over
//     gridDim.y, so B = 1, N = 10000, M = 20000 is 10 x 40 workgroups; the per-(tile, query) minima go to the workspace
//     as partial[b][tile][query].
//   * uhd_query_kernel: a lane per query takes the minimum over the tiles and remembers the LOWEST tile that attains it
//     (strict <, tiles ascending); the workgroup then keeps its greatest minimum, the lowest query index among equals.
//   * uhd_finish_kernel: one workgroup per batch element reduces those per-workgroup records the same way to (d2, i*),
//     then re-evaluates query i* against the kUhdTile targets of its tile -- the same operations give the same bits -- and
//     takes the lowest j whose s equals d2.  That is numpy's argmax over argmin, judged on s.
// A pair whose s is NaN is skipped by fmin; see include/genpc_hip.h for what non-finite input returns.
// Everything is enqueued on the caller's stream; nothing is read back.
#include "uhd.h"
#include "../../include/genpc_hip.h"

namespace genpc {

__global__ __launch_bounds__(kUhdBlock) void uhd_pairs_kernel(int n, const float *__restrict__ xyz, int m, const float *__restrict__ xyz2,
                                                              double *__restrict__ partial)
{
    __shared__ double s_t[kUhdTile * 3];
    const int batch = blockIdx.z, tile = blockIdx.y, tiles = gridDim.y;
    const int j0 = tile * kUhdTile, cnt = min(kUhdTile, m - j0);
    const float *__restrict__ T = xyz2 + ((size_t)batch * m + j0) * 3;
    for (int k = threadIdx.x; k < cnt * 3; k += kUhdBlock) s_t[k] = (double)T[k];
    __syncthreads();
    const int i0 = blockIdx.x * (kUhdBlock * kUhdQ) + threadIdx.x;
    const float *__restrict__ Q = xyz + (size_t)batch * n * 3;
    double qx[kUhdQ], qy[kUhdQ], qz[kUhdQ], best[kUhdQ];
#pragma unroll
    for (int q = 0; q < kUhdQ; q++) {
        const int i = min(i0 + q * kUhdBlock, n - 1);          // lanes past the end redo the last query and store nothing
        qx[q] = (double)Q[(size_t)i * 3 + 0];
        qy[q] = (double)Q[(size_t)i * 3 + 1];
        qz[q] = (double)Q[(size_t)i * 3 + 2];
        best[q] = __builtin_inf();
    }
#pragma unroll 4
    for (int j = 0; j < cnt; j++) {
        const double tx = s_t[j * 3 + 0], ty = s_t[j * 3 + 1], tz = s_t[j * 3 + 2];
#pragma unroll
        for (int q = 0; q < kUhdQ; q++) best[q] = fmin(best[q], uhd_s(qx[q], qy[q], qz[q], tx, ty, tz));
    }
    double *__restrict__ P = partial + ((size_t)batch * tiles + tile) * n;
#pragma unroll
    for (int q = 0; q < kUhdQ; q++) {
        const int i = i0 + q * kUhdBlock;
        if (i < n) P[i] = best[q];
    }
}

__global__ __launch_bounds__(kUhdBlock) void uhd_query_kernel(int n, int tiles, const double *__restrict__ partial, UhdRec *__restrict__ recs)
{
    __shared__ UhdRec s_r[kUhdBlock];
    const int batch = blockIdx.y, i = blockIdx.x * kUhdBlock + threadIdx.x;
    UhdRec r{-1.0, kUhdNoIndex, 0};                    // below every minimum (s >= 0)
    if (i < n) {
        const double *__restrict__ P = partial + (size_t)batch * tiles * n + i;
        double v = P[0];
        int tile = 0;
        for (int t = 1; t < tiles; t++) {
            const double p = P[(size_t)t * n];
            if (p < v) { v = p; tile = t; }
        }
        r = UhdRec{v, i, tile};
    }
    r = uhd_block_best(r, s_r);
    if (threadIdx.x == 0) recs[(size_t)batch * gridDim.x + blockIdx.x] = r;
}

__global__ __launch_bounds__(kUhdBlock) void uhd_finish_kernel(int n, const float *__restrict__ xyz, int m, const float *__restrict__ xyz2,
                                                               int nrecs, const UhdRec *__restrict__ recs, double *__restrict__ out_d2,
                                                               int *__restrict__ out_ij)
{
    __shared__ UhdRec s_r[kUhdBlock];
    __shared__ int s_j[kUhdBlock];
    const int batch = blockIdx.x;
    UhdRec r{-1.0, kUhdNoIndex, 0};
    for (int k = threadIdx.x; k < nrecs; k += kUhdBlock) {
        const UhdRec o = recs[(size_t)batch * nrecs + k];
        if (uhd_beats(o.v, o.i, r.v, r.i)) r = o;
    }
    r = uhd_block_best(r, s_r);
    const float *qp = xyz + ((size_t)batch * n + min(r.i, n - 1)) * 3;      // (r.i is a query index: every workgroup had one)
    const double qx = (double)qp[0], qy = (double)qp[1], qz = (double)qp[2];
    const int j0 = r.tile * kUhdTile, cnt = min(kUhdTile, m - j0);
    int jbest = kUhdNoIndex;
    for (int k = threadIdx.x; k < cnt; k += kUhdBlock) {          // ascending per thread: the first hit is the thread's lowest
        const float *tp = xyz2 + ((size_t)batch * m + j0 + k) * 3;
        if (jbest == kUhdNoIndex && uhd_s(qx, qy, qz, (double)tp[0], (double)tp[1], (double)tp[2]) == r.v) jbest = j0 + k;
    }
    s_j[threadIdx.x] = jbest;
    __syncthreads();
    for (int w = kUhdBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s_j[threadIdx.x] = min(s_j[threadIdx.x], s_j[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out_d2[batch] = r.v;
        out_ij[batch * 2 + 0] = r.i;
        out_ij[batch * 2 + 1] = s_j[0] == kUhdNoIndex ? -1 : s_j[0];
    }
}

static int uhd(int b, int n, const float *xyz, int m, const float *xyz2, double *out_d2, int *out_ij, hipStream_t st)
{
    const int tiles = ceil_div(m, kUhdTile), qblocks = ceil_div(n, kUhdBlock * kUhdQ), nrecs = ceil_div(n, kUhdBlock);
    if (tiles > 65535 || b > 65535 || n > (1 << 30)) {
        set_error("genpc_uhd: problem too large for one launch (B <= 65535, N <= 2^30, M <= 65535 * 512)");
        return -1;
    }
    double *partial; UhdRec *recs;
    WsLayout L;
    L.add(partial, (size_t)b * tiles * n);
    L.add(recs, (size_t)b * nrecs);
    if (!ws_alloc(L, kWsUhd, st)) return -1;
    hipLaunchKernelGGL(uhd_pairs_kernel, dim3(qblocks, tiles, b), dim3(kUhdBlock), 0, st, n, xyz, m, xyz2, partial);
    if (!check(hipGetLastError(), "uhd_pairs_kernel launch")) return -1;
    hipLaunchKernelGGL(uhd_query_kernel, dim3(nrecs, b), dim3(kUhdBlock), 0, st, n, tiles, (const double *)partial, recs);
    if (!check(hipGetLastError(), "uhd_query_kernel launch")) return -1;
    hipLaunchKernelGGL(uhd_finish_kernel, dim3(b), dim3(kUhdBlock), 0, st, n, xyz, m, xyz2, nrecs, (const UhdRec *)recs, out_d2, out_ij);
    return check(hipGetLastError(), "uhd_finish_kernel launch") ? 0 : -1;
}

}  // namespace genpc

GENPC_API int genpc_uhd(int b, int n, const float *xyz, int m, const float *xyz2, double *out_d2, int *out_ij, void *stream)
{
    using namespace genpc;
    if (b < 0) {
        set_error("genpc_uhd: negative batch size");
        return -1;
    }
    if (b == 0) return 1;
    if (n <= 0 || m <= 0) {
        set_error("genpc_uhd: the maximum or minimum of an empty set is undefined (n and m must be positive)");
        return -1;
    }
    if (!xyz || !xyz2 || !out_d2 || !out_ij) {
        set_error("genpc_uhd: null pointer");
        return -1;
    }
    return uhd(b, n, xyz, m, xyz2, out_d2, out_ij, (hipStream_t)stream);
}
