// fps_plan_check -- csrc/fps_plan.h by itself (plain C++, built with the address and undefined-behaviour sanitizers by
// tests/test_fps_plan.py): the three ranges and their boundaries, force_large, the refusals, every workspace count monotone
// in n, and every packed field of the large sampler holding its maximum at the limit.
#include "fps_plan.h"

#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>

using namespace genpc;

static int g_fail = 0;
#define EXPECT(cond)                                                            \
    do {                                                                        \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); g_fail++; } \
    } while (0)

int main(int argc, char **argv)
{
    // with arguments: print the plan of (n, force_large) as genpc_fps_plan lays it out (the Python side compares)
    if (argc == 3) {
        const FpsPlan p = fps_plan(atoi(argv[1]), atoi(argv[2]));
        printf("%d %d %d %d %d %d %d %d\n", p.sampler, p.cells_max, p.cells_target, p.npad, p.chunks, p.starts, p.lds_bytes, p.build_own);
        return 0;
    }
    // the three ranges and their boundaries
    EXPECT(fps_plan(1, 0).sampler == kFpsGrid);
    EXPECT(fps_plan(24576, 0).sampler == kFpsGrid);
    EXPECT(fps_plan(24577, 0).sampler == kFpsMulti);
    EXPECT(fps_plan(262144, 0).sampler == kFpsMulti);
    EXPECT(fps_plan(262145, 0).sampler == kFpsLarge);
    EXPECT(fps_plan(4194304, 0).sampler == kFpsLarge);
    EXPECT(kFpsGridMaxN == 24576 && kFpsMultiMaxN == 262144 && kFpsLargeMaxN == 4194304);
    // nothing but the sampler for the two that size themselves
    for (int n : {1, 24576, 24577, 262144}) {
        const FpsPlan p = fps_plan(n, 0);
        EXPECT(p.cells_max == 0 && p.cells_target == 0 && p.npad == 0 && p.chunks == 0 && p.starts == 0 && p.lds_bytes == 0);
    }
    // force_large: any size
    for (int n : {1, 2, 63, 24576, 24577, 262144, 262145, 4194304}) {
        const FpsPlan p = fps_plan(n, 1);
        EXPECT(p.sampler == kFpsLarge);
        EXPECT(p.npad >= n && p.npad % kFpsLargePad == 0 && p.npad - n < kFpsLargePad);
        EXPECT(p.chunks * kFpsLargeChunk == p.npad && p.chunks % 4 == 0);
        EXPECT(p.cells_target >= 1 && p.cells_target <= p.cells_max && p.starts == p.cells_max + 1);
        EXPECT(p.lds_bytes == (int)kFpsLargeLdsBytes && p.lds_bytes <= 64 * 1024 && p.build_own == 0);
    }
    EXPECT(fps_plan(1, 1).npad == 128 && fps_plan(1, 1).chunks == 16 && fps_plan(1, 1).cells_target == 64);
    EXPECT(fps_plan(262145, 0).npad == 262272 && fps_plan(262145, 0).cells_target == 12288);
    // refusals
    for (int force = 0; force < 2; force++) {
        EXPECT(fps_plan(0, force).sampler == kFpsNone);
        EXPECT(fps_plan(-5, force).sampler == kFpsNone);
        EXPECT(fps_plan(4194305, force).sampler == kFpsNone);
        EXPECT(fps_plan(2147483647, force).sampler == kFpsNone);
        EXPECT(fps_plan(4194305, force).npad == 0 && fps_plan(4194305, force).lds_bytes == 0);
    }
    // every workspace count is monotone in n (every n near a boundary of the padding, strides elsewhere)
    FpsPlan prev = fps_plan(1, 1);
    for (int n = 2; n <= kFpsLargeMaxN; n += (n < 70000 || n > kFpsLargeMaxN - 70000) ? 1 : 997) {
        const FpsPlan p = fps_plan(n, 1);
        EXPECT(p.npad >= prev.npad && p.chunks >= prev.chunks && p.cells_target >= prev.cells_target && p.cells_max >= prev.cells_max);
        EXPECT(p.starts >= prev.starts && p.lds_bytes >= prev.lds_bytes);
        if (g_fail) break;
        prev = p;
    }
    // every packed field holds its maximum at the limit
    {
        const FpsPlan p = fps_plan(kFpsLargeMaxN, 1);
        const unsigned long long last_pos = (unsigned long long)p.npad - 1, last_index = (unsigned long long)kFpsLargeMaxN - 1;
        EXPECT(last_pos < (1ull << kFpsLargePosBits));
        EXPECT(last_index < (1ull << kFpsLargeIndexBits));
        const unsigned long long key = (last_index << kFpsLargePosBits) | last_pos;
        EXPECT((key >> kFpsLargePosBits) == last_index && (key & ((1ull << kFpsLargePosBits) - 1)) == last_pos);
        EXPECT((long long)key >= 0);
        const unsigned last_cell = (unsigned)p.cells_max - 1, last_sample = (unsigned)kFpsLargePick - 1;
        const unsigned long long item = ((unsigned long long)last_sample << kFpsLargeCellBits) | last_cell;
        EXPECT(item <= 0xffffffffull);
        EXPECT((unsigned)(item >> kFpsLargeCellBits) == last_sample && ((unsigned)item & ((1u << kFpsLargeCellBits) - 1u)) == last_cell);
        EXPECT((long long)p.npad * 16 < (1ll << 31) * 16 && (long long)p.chunks * 4 == p.npad / 2);
        EXPECT(p.cells_max < (1 << 19));
    }
    if (g_fail) return 1;
    printf("fps_plan_check: ok\n");
    return 0;
}
