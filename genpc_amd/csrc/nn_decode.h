// nn_decode.h -- which (query block, batch element, slice) a block of a nearest-neighbour launch is, and which (batch element,
// 64-query block) a finish block is: the division of a block id by divisors that are the same for every block of a launch.
// The host computes a multiplier and a shift per divisor where it fills NNArgs (nn_forward, launch_nn_finish); the kernels
// (nn_forward_kernel, nn_mfma_kernel, nn_f16_kernel, nn_finish_kernel) divide with one multiply-high and one shift -- a
// runtime integer division is ~25 scalar instructions through v_rcp_iflag_f32, and it stood between the kernel arguments and
// the first load of every block.  Host and device code, no HIP header needed: tests/nn_decode_check.cpp includes it as plain
// C++ and compares it with / and %.
#pragma once
#include "nn_plan.h"      // kFQ

#if defined(__HIPCC__)
#define GENPC_HD __host__ __device__ __forceinline__
#else
#define GENPC_HD inline
#endif

namespace genpc {

// n / d for 0 <= n < 2^31 and 1 <= d < 2^31:  l = ceil(log2 d), mul = ceil(2^(31 + l) / d) < 2^32, and
//     n / d = (mul * n) >> (31 + l) = mulhi(2 n, mul) >> l
// (Granlund & Montgomery 1994, theorem 4.2 with N = 31: 2^(N+l) <= mul * d <= 2^(N+l) + 2^l holds because mul * d exceeds
// 2^(N+l) by less than d <= 2^l.  mul < 2^32: d = 2^l gives 2^31; otherwise d >= 2^(l-1) + 1 and 2^(31+l) / d < 2^32 - 1 for
// l <= 31.)  Block ids are below 2^31 (nn_plan's too_large), so 2 n fits 32 bits.
struct NNDiv {
    unsigned mul, shift;
};

inline NNDiv nn_div_make(int d)
{
    NNDiv v{0u, 0u};
    if (d < 1) return v;                  // (a direction that is not there: never divided by)
    unsigned l = 0;
    while (((unsigned long long)1 << l) < (unsigned long long)d) l++;
    v.mul = (unsigned)((((unsigned long long)1 << (31 + l)) + (unsigned long long)d - 1) / (unsigned long long)d);
    v.shift = l;
    return v;
}

GENPC_HD int nn_div(int n, NNDiv v)
{
    return (int)((unsigned)(((unsigned long long)((unsigned)n << 1) * v.mul) >> 32) >> v.shift);
}

// finish blocks per batch element of a direction with nq queries
GENPC_HD int nn_fin_blocks(int nq) { return (nq + kFQ - 1) / kFQ; }

// block id within its direction = (slice * b + batch) * qblocks + qb
struct NNBlockId {
    int qb, batch, slice;
};

GENPC_HD NNBlockId nn_decode_block(int bid, int qblocks, NNDiv by_qblocks, int b, NNDiv by_b)
{
    NNBlockId k;
    const int rest = nn_div(bid, by_qblocks);
    k.qb = bid - rest * qblocks;
    k.slice = nn_div(rest, by_b);
    k.batch = rest - k.slice * b;
    return k;
}

// finish block id within its direction = batch * fblocks + fb
struct NNFinId {
    int batch, fb;
};

GENPC_HD NNFinId nn_decode_fin(int bid, int fblocks, NNDiv by_fblocks)
{
    NNFinId k;
    k.batch = nn_div(bid, by_fblocks);
    k.fb = bid - k.batch * fblocks;
    return k;
}

// every stride-th block of a launch (the finish step's sampled report)
GENPC_HD bool nn_is_multiple(int bid, int stride, NNDiv by_stride) { return bid - nn_div(bid, by_stride) * stride == 0; }

}  // namespace genpc
