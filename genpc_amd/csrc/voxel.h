// voxel.h -- what voxel.hip (one cloud) and voxel_ragged.hip (many clouds, one call) state once: the order-preserving map of a
// float onto an unsigned int, under which the bounds are folded with integer atomics, and a point's 63-bit voxel key.
#pragma once
#include "common.h"

namespace genpc {

constexpr int kVBlock = 256;

__device__ __forceinline__ unsigned f2ord(float f)      // order-preserving map float -> uint
{
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned o)
{
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// key = i << 42 | j << 21 | k of the point p[3] in the grid anchored at the cloud's minimum (bmin[3], ordered uints) minus half
// a voxel, every step in double.  False, and key = ~0: a non-finite coordinate, or a grid finer than 2^21 cells on an axis.
__device__ __forceinline__ bool voxel_point_key(const float *__restrict__ p, double voxel, const unsigned *__restrict__ bmin,
                                                unsigned long long &key)
{
    key = 0ull;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double origin = (double)ord2f(bmin[k]) - voxel * 0.5;
        const double c = floor(((double)p[k] - origin) / voxel);
        if (!(c >= 0.0 && c < 2097152.0)) { key = ~0ull; return false; }
        key = (key << 21) | (unsigned long long)c;
    }
    return true;
}

}  // namespace genpc
