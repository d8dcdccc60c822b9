// uhd.h -- what uhd.hip (rectangular batch) and uhd_ragged.hip (ragged batch) share: the launch constants, the one fp64
// squared distance both evaluate, the order among candidate witnesses and the workgroup's reduction under it.  The bit-exact
// tests of both rest on these being one definition.
#pragma once
#include "common.h"

namespace genpc {

constexpr int kUhdBlock = 256;
constexpr int kUhdQ = 4;                          // queries per lane
constexpr int kUhdTile = 512;                     // targets per workgroup: 12 KiB of LDS as doubles
constexpr int kUhdNoIndex = 0x7fffffff;

struct UhdRec {                                   // a candidate witness: query i, its minimum v, the lowest tile that attains it
    double v;
    int i, tile;
};

// a beats b: the greater minimum, among equals the lower query index (minima are never NaN: fmin drops them)
__device__ __forceinline__ bool uhd_beats(double av, int ai, double bv, int bi) { return av > bv || (av == bv && ai < bi); }

__device__ __forceinline__ double uhd_s(double qx, double qy, double qz, double tx, double ty, double tz)
{
    const double dx = qx - tx, dy = qy - ty, dz = qz - tz;
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// the workgroup's best record, returned to every thread (s_r: kUhdBlock records of scratch)
__device__ __forceinline__ UhdRec uhd_block_best(UhdRec r, UhdRec *s_r)
{
    s_r[threadIdx.x] = r;
    __syncthreads();
    for (int w = kUhdBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const UhdRec o = s_r[threadIdx.x + w];
            if (uhd_beats(o.v, o.i, s_r[threadIdx.x].v, s_r[threadIdx.x].i)) s_r[threadIdx.x] = o;
        }
        __syncthreads();
    }
    return s_r[0];
}

}  // namespace genpc
