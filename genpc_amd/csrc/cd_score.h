// cd_score.h -- the ONE statement of the scale search's score (reg_xyz.py:81-83,167-169) and of the order of its sums:
//   score = float(sum64 sqrtf(d1) / n1) + float(sum64 sqrtf(d2) / n2) * w
// by a workgroup of kIBlock threads: thread t adds the points t, t + kIBlock, ... in that order (cd_score_thread_sum), the 64
// lanes of a wave are added by an xor butterfly (32, 16, ... 1), the waves 0 ... 3 by thread 0, which divides and writes.
// cd_score_kernel (icp.hip: the distances come from arrays) and scale_search_ragged_kernel (scale_search_ragged.hip: every
// distance is searched where it is added) are both this and nothing else, which is what makes their scores the same bits.
#pragma once
#include "common.h"

namespace genpc {

constexpr int kIBlock = 256;

// the calling thread's share of sum sqrtf(d2(j)), j < n: d2(j) is the squared distance of point j
template <typename D2>
__device__ __forceinline__ double cd_score_thread_sum(int n, D2 d2)
{
    double a = 0.0;
    for (int j = threadIdx.x; j < n; j += kIBlock) a += (double)sqrtf(d2(j));
    return a;
}

// a, b: every thread's shares of the two sums; red: 2 * kIBlock / kWave doubles of LDS that nobody else uses meanwhile.
// Thread 0 writes *score.  (One barrier inside: the whole workgroup calls.)
__device__ __forceinline__ void cd_score_reduce(double a, double b, int n1, int n2, float w, double *red, float *score)
{
    constexpr int kWaves = kIBlock / kWave;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_xor(a, off, kWave);
        b += __shfl_xor(b, off, kWave);
    }
    if (lane == 0) {
        red[wave] = a;
        red[kWaves + wave] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double x = 0.0, y = 0.0;
        for (int q = 0; q < kWaves; q++) {
            x += red[q];
            y += red[kWaves + q];
        }
        const float m1 = (float)(x / n1), m2 = (float)(y / n2);
        *score = m1 + m2 * w;
    }
}

}  // namespace genpc
