// hpr_order.hip -- hidden-point removal, the ordering pass (hpr.hip describes the whole): later copies of exact duplicates are
// marked, every view's points are put in 2-D Morton order of their DIRECTION from the eye, flipped, and summarised per tile of
// 128 consecutive positions.
#include "hpr.h"

#include <algorithm>
#include <rocprim/device/device_radix_sort.hpp>

namespace genpc {

// p' for every (view, point), stored in Morton order (row pos = point perm[pos]); open3d: |v| = 0 -> 1e-4
__global__ __launch_bounds__(256) void hpr_flip_kernel(int n, const float *__restrict__ pts, const int *__restrict__ perm,
                                                      const double *__restrict__ eyes, double radius, double *__restrict__ fl,
                                                      const unsigned char *__restrict__ dup)
{
    const int pos = blockIdx.x * 256 + threadIdx.x, view = blockIdx.y;
    if (pos >= n) return;
    const int i = perm[(size_t)view * n + pos];
    if (dup[i]) {
        // a later copy of an exact duplicate: NaN -- hidden, and it cuts nothing (its lowest-index twin stands for both)
        double *o = fl + ((size_t)view * n + pos) * 3;
        o[0] = o[1] = o[2] = __builtin_nan("");
        return;
    }
    const double vx = (double)pts[(size_t)i * 3 + 0] - eyes[view * 3 + 0];
    const double vy = (double)pts[(size_t)i * 3 + 1] - eyes[view * 3 + 1];
    const double vz = (double)pts[(size_t)i * 3 + 2] - eyes[view * 3 + 2];
    double r = sqrt(vx * vx + vy * vy + vz * vz);
    if (r == 0.0) r = 0.0001;
    const double k = 2.0 * (radius - r) / r;
    double *o = fl + ((size_t)view * n + pos) * 3;
    o[0] = vx + k * vx;
    o[1] = vy + k * vy;
    o[2] = vz + k * vz;
}

// Exact duplicates.  qhull (open3d's hidden_point_removal) reports ONE copy of a group of coincident points as a hull
// vertex -- which one is its own business -- so only the copy with the lowest index takes part here: three stable
// radix sorts (z, y, x keys; -0 counts as +0) order the points lexicographically with the index as the last key, and a
// point equal to its predecessor is a later copy.
__global__ __launch_bounds__(256) void hpr_dupkey_kernel(int n, const float *__restrict__ pts, int axis, const int *__restrict__ order,
                                                        unsigned *__restrict__ keys, int *__restrict__ idx)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int i = order ? order[p] : p;
    keys[p] = hpr_ord(pts[(size_t)i * 3 + axis] + 0.0f);
    if (!order) idx[p] = p;
}
__global__ __launch_bounds__(256) void hpr_dupmark_kernel(int n, const float *__restrict__ pts, const int *__restrict__ order,
                                                         unsigned char *__restrict__ dup)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int i = order[p];
    bool d = false;
    if (p > 0) {
        const int j = order[p - 1];
        d = pts[(size_t)i * 3 + 0] == pts[(size_t)j * 3 + 0] && pts[(size_t)i * 3 + 1] == pts[(size_t)j * 3 + 1] &&
            pts[(size_t)i * 3 + 2] == pts[(size_t)j * 3 + 2];
    }
    dup[i] = d ? 1 : 0;
}

// bounds[0..2] = min, [3..5] = max of the finite coordinates, as ordered uints (0xffffffff / 0 initially)
__global__ __launch_bounds__(256) void hpr_bounds_kernel(int n, const float *__restrict__ pts, unsigned *bounds)
{
    unsigned mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float v = pts[(size_t)i * 3 + k];
            if (!(fabsf(v) < __builtin_inff())) continue;
            const unsigned o = hpr_ord(v);
            mn[k] = o < mn[k] ? o : mn[k];
            mx[k] = o > mx[k] ? o : mx[k];
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned a = (unsigned)__shfl_xor((int)mn[k], off, kWave), b = (unsigned)__shfl_xor((int)mx[k], off, kWave);
            mn[k] = a < mn[k] ? a : mn[k];
            mx[k] = b > mx[k] ? b : mx[k];
        }
        if ((threadIdx.x & (kWave - 1)) == 0) {
            atomicMin(&bounds[k], mn[k]);
            atomicMax(&bounds[3 + k], mx[k]);
        }
    }
}

__device__ __forceinline__ unsigned hpr_spread10(unsigned v)      // 10 bits -> every second bit
{
    v = (v | (v << 8)) & 0x00ff00ffu;
    v = (v | (v << 4)) & 0x0f0f0f0fu;
    v = (v | (v << 2)) & 0x33333333u;
    v = (v | (v << 1)) & 0x55555555u;
    return v;
}

__device__ __forceinline__ HprViewFrame hpr_view_frame(const unsigned *bounds, const double *eye)
{
    const double lx = (double)hpr_unord(bounds[0]), ly = (double)hpr_unord(bounds[1]), lz = (double)hpr_unord(bounds[2]);
    const double hx = (double)hpr_unord(bounds[3]), hy = (double)hpr_unord(bounds[4]), hz = (double)hpr_unord(bounds[5]);
    double wx = (lx + hx) * 0.5 - eye[0], wy = (ly + hy) * 0.5 - eye[1], wz = (lz + hz) * 0.5 - eye[2];
    const double dist = sqrt(wx * wx + wy * wy + wz * wz);
    const double hd = 0.5 * sqrt((hx - lx) * (hx - lx) + (hy - ly) * (hy - ly) + (hz - lz) * (hz - lz));
    HprViewFrame v;
    if (dist > 0.0 && dist < __builtin_inf()) { wx /= dist; wy /= dist; wz /= dist; }
    else { wx = 0.0; wy = 0.0; wz = 1.0; }
    const double ax = fabs(wx), ay = fabs(wy), az = fabs(wz);
    double x, y, z;
    if (ax <= ay && ax <= az) { x = 0.0; y = wz; z = -wy; }
    else if (ay <= az)        { x = -wz; y = 0.0; z = wx; }
    else                      { x = wy; y = -wx; z = 0.0; }
    const double l = sqrt(x * x + y * y + z * z);
    v.e1x = x / l; v.e1y = y / l; v.e1z = z / l;
    v.e2x = wy * v.e1z - wz * v.e1y;
    v.e2y = wz * v.e1x - wx * v.e1z;
    v.e2z = wx * v.e1y - wy * v.e1x;
    double s = 1.0;
    if (dist > hd) {
        s = 1.05 * hd / dist;
        s = s < 1.0 ? s : 1.0;
    }
    v.s = s > 0.0 ? s : 1.0;
    return v;
}

// Sort key of (view, point): view << 20 | 2-D Morton code of the point's DIRECTION from the eye, 10 bits per
// axis over [-s, s]^2 (non-finite points last within their view).  Points that lie in the same direction --
// a front surface and what it hides -- become neighbours; the order has no influence on the result.
__global__ __launch_bounds__(256) void hpr_key_kernel(int n, const float *__restrict__ pts, const unsigned *__restrict__ bounds,
                                                     const double *__restrict__ eyes, unsigned *__restrict__ keys, int *__restrict__ idx)
{
    const int i = blockIdx.x * 256 + threadIdx.x, view = blockIdx.y;
    if (i >= n) return;
    const HprViewFrame V = hpr_view_frame(bounds, eyes + view * 3);
    const double vx = (double)pts[(size_t)i * 3 + 0] - eyes[view * 3 + 0];
    const double vy = (double)pts[(size_t)i * 3 + 1] - eyes[view * 3 + 1];
    const double vz = (double)pts[(size_t)i * 3 + 2] - eyes[view * 3 + 2];
    const double r = sqrt(vx * vx + vy * vy + vz * vz);
    unsigned key = 0xfffffu;
    if (r > 0.0 && r < __builtin_inf()) {
        const double dx = vx / r, dy = vy / r, dz = vz / r;
        const double x = dx * V.e1x + dy * V.e1y + dz * V.e1z;
        const double y = dx * V.e2x + dy * V.e2y + dz * V.e2z;
        double qx = floor((x / V.s + 1.0) * 512.0), qy = floor((y / V.s + 1.0) * 512.0);
        qx = qx < 0.0 ? 0.0 : (qx > 1023.0 ? 1023.0 : qx);
        qy = qy < 0.0 ? 0.0 : (qy > 1023.0 ? 1023.0 : qy);
        key = hpr_spread10((unsigned)qx) | (hpr_spread10((unsigned)qy) << 1);
    }
    keys[(size_t)view * n + i] = ((unsigned)view << 20) | key;
    idx[(size_t)view * n + i] = i;
}

__global__ __launch_bounds__(kHprThreads) void hpr_tile_kernel(int n, const double *__restrict__ fl_all, HprTile *__restrict__ tiles)
{
    __shared__ double red[4][kHprThreads];
    const int view = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const int pos = tile * kHprThreads + tid;
    double ux = 0.0, uy = 0.0, uz = 0.0, rho = 0.0;
    bool ok = false;
    if (pos < n) {
        const double *p = fl_all + ((size_t)view * n + pos) * 3;
        rho = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
        ok = rho > 0.0 && rho < __builtin_inf();
        if (ok) { ux = p[0] / rho; uy = p[1] / rho; uz = p[2] / rho; }
        else rho = 0.0;
    }
    red[0][tid] = ux; red[1][tid] = uy; red[2][tid] = uz; red[3][tid] = rho;
    __syncthreads();
    for (int h = kHprThreads / 2; h > 0; h >>= 1) {
        if (tid < h) {
            red[0][tid] += red[0][tid + h];
            red[1][tid] += red[1][tid + h];
            red[2][tid] += red[2][tid + h];
            red[3][tid] = red[3][tid] > red[3][tid + h] ? red[3][tid] : red[3][tid + h];
        }
        __syncthreads();
    }
    const double sx = red[0][0], sy = red[1][0], sz = red[2][0], rho_max = red[3][0];
    const double l = sqrt(sx * sx + sy * sy + sz * sz);
    __syncthreads();
    const bool axis = l > 0.0 && rho_max > 0.0;
    const double wx = axis ? sx / l : 0.0, wy = axis ? sy / l : 0.0, wz = axis ? sz / l : 0.0;
    red[0][tid] = ok ? ux * wx + uy * wy + uz * wz : 1.0;
    __syncthreads();
    for (int h = kHprThreads / 2; h > 0; h >>= 1) {
        if (tid < h) red[0][tid] = red[0][tid] < red[0][tid + h] ? red[0][tid] : red[0][tid + h];
        __syncthreads();
    }
    if (tid == 0) {
        HprTile t;
        double c = red[0][0] - 1e-12;          // widen the cone past roundoff
        if (!axis) c = -1.0;                   // no usable axis: never skipped
        t.wx = wx; t.wy = wy; t.wz = wz;
        t.cos_phi = c;
        t.cos2_phi = c * c;
        t.sin2_phi = 1.0 - c * c + 1e-15;
        t.sin_phi = sqrt(t.sin2_phi) * (1.0 + 1e-15);
        t.inv_rho_max = rho_max > 0.0 ? 1.0 / (rho_max * (1.0 + 1e-12)) : 0.0;
        tiles[(size_t)view * gridDim.x + tile] = t;
    }
}

bool hpr_sort_bytes(size_t pairs, hipStream_t stream, size_t &bytes)
{
    bytes = 0;
    return check(rocprim::radix_sort_pairs(nullptr, bytes, (const unsigned *)nullptr, (unsigned *)nullptr, (const int *)nullptr, (int *)nullptr,
                                           pairs, 0u, 32u, stream),
                 "hpr sort size");
}

bool hpr_launch_order(const HprPlan &plan, const HprCall &k, hipStream_t stream)
{
    const int n = k.n, c = k.c, g256 = plan.row_grid;
    size_t sort_bytes = k.sort_bytes;
    // later copies of exact duplicates (the key / index buffers of the view sort are free until then)
    {
        int *ia = k.i0, *ib = k.i1;
        for (int axis = 2; axis >= 0; axis--) {
            hipLaunchKernelGGL(hpr_dupkey_kernel, dim3(g256), dim3(256), 0, stream, n, k.points, axis, axis == 2 ? (const int *)nullptr : (const int *)ia, k.k0, ia);
            size_t sb = sort_bytes;
            if (!check(rocprim::radix_sort_pairs(k.sort_tmp, sb, (const unsigned *)k.k0, k.k1, (const int *)ia, ib, (size_t)n, 0u, 32u, stream), "hpr duplicate sort"))
                return false;
            std::swap(ia, ib);
        }
        hipLaunchKernelGGL(hpr_dupmark_kernel, dim3(g256), dim3(256), 0, stream, n, k.points, (const int *)ia, k.dup);
    }
    hipLaunchKernelGGL(hpr_bounds_kernel, dim3(plan.bounds_grid), dim3(256), 0, stream, n, k.points, k.bounds());
    hipLaunchKernelGGL(hpr_key_kernel, dim3(g256, c), dim3(256), 0, stream, n, k.points, (const unsigned *)k.bounds(), k.eyes, k.k0, k.i0);
    if (!check(rocprim::radix_sort_pairs(k.sort_tmp, sort_bytes, (const unsigned *)k.k0, k.k1, (const int *)k.i0, k.i1, (size_t)plan.pairs, 0u, (unsigned)plan.key_bits, stream),
               "hpr radix sort"))
        return false;
    hipLaunchKernelGGL(hpr_flip_kernel, dim3(g256, c), dim3(256), 0, stream, n, k.points, (const int *)k.i1, k.eyes, k.radius, k.fl, (const unsigned char *)k.dup);
    hipLaunchKernelGGL(hpr_tile_kernel, dim3(plan.ntiles, c), dim3(kHprThreads), 0, stream, n, (const double *)k.fl, k.tiles);
    return true;
}

}  // namespace genpc
