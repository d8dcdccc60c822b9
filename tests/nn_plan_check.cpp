// Stand-alone check of genpc_amd/csrc/nn_plan.h (host code only; tests/test_nn_plan.py builds it with
// -fsanitize=address,undefined and runs it).  Exit status 0 = every check passed; each failure prints what it found.
// The table holds asks and the plans they must give as literals, no second copy of the header's expressions; the properties
// below it are checked over a sweep of shapes, CU counts and families.
// `nn_plan_check --exported` prints, for the rows that genpc_nn_plan can be asked (both directions each other's swap or one
// direction, no radius, no switch set), "b n m ndir cus forced : the sixteen values of out[]" from the table's literals.
#include "nn_plan.h"

#include <stdio.h>
#include <string.h>

using namespace genpc;

static int g_failed = 0;
static bool g_print = false;

struct Ask {
    int b, ndir, nq[2], nt[2], swapped, radius, cus, forced, env_family, env_r, env_q, env_u, env_wps;
};
struct Want {
    int family, form, r, q, unit, nl, slice_len, qblocks[2], slices[2], block_begin[2], unit_begin[2], fin_begin[2];
    long long blocks, units;
    int pwords;
    long long part_words, fin_blocks;
    int hint_stride, early, too_large;
};

static NNAsk ask_of(const Ask &k)
{
    NNAsk a;
    a.b = k.b;
    a.ndir = k.ndir;
    for (int d = 0; d < 2; d++) { a.nq[d] = k.nq[d]; a.nt[d] = k.nt[d]; }
    a.swapped = k.swapped != 0;
    a.radius = k.radius != 0;
    a.cus = k.cus;
    a.forced = k.forced;
    a.env_family = k.env_family;
    a.env_r = k.env_r;
    a.env_q = k.env_q;
    a.env_u = k.env_u;
    a.env_wps = k.env_wps;
    return a;
}

static const char *g_row = "";
static void expect(const char *what, long long got, long long want)
{
    if (got != want) { printf("FAILED row '%s': %s = %lld, expected %lld\n", g_row, what, got, want); g_failed++; }
}

static void row(const char *label, const Ask &k, const Want &w)
{
    g_row = label;
    if (g_print) {
        const bool shaped = k.ndir == 1 || (k.ndir == 2 && k.swapped && k.nq[1] == k.nt[0] && k.nt[1] == k.nq[0]);
        if (!shaped || k.radius || k.env_family != -1 || k.env_r || k.env_q || k.env_u || k.env_wps) return;
        const long long big = 0x7fffffff;
        printf("%d %d %d %d %d %d : %d %d %d %d %d %d %d %d %lld %lld %d %d %d %d %d %d\n", k.b, k.nq[0], k.nt[0], k.ndir, k.cus, k.forced, w.family, w.form,
               w.family == kNNValu ? w.r : w.q, w.unit, w.nl, w.slice_len, w.slices[0], w.slices[1], w.blocks < big ? w.blocks : big,
               w.fin_blocks < big ? w.fin_blocks : big, w.early, w.too_large, w.qblocks[0], w.qblocks[1], w.hint_stride, k.cus);
        return;
    }
    const NNPlan p = nn_plan(ask_of(k));
    expect("family", p.family, w.family);
    expect("form", p.form, w.form);
    expect("r", p.r, w.r);
    expect("q", p.q, w.q);
    expect("unit", p.unit, w.unit);
    expect("nl", p.nl, w.nl);
    expect("slice_len", p.slice_len, w.slice_len);
    for (int d = 0; d < 2; d++) {
        expect("qblocks", p.dir[d].qblocks, w.qblocks[d]);
        expect("slices", p.dir[d].slices, w.slices[d]);
        expect("block_begin", p.dir[d].block_begin, w.block_begin[d]);
        expect("unit_begin", p.dir[d].unit_begin, w.unit_begin[d]);
        expect("fin_begin", p.dir[d].fin_begin, w.fin_begin[d]);
    }
    expect("blocks", p.blocks, w.blocks);
    expect("units", p.units, w.units);
    expect("pwords", p.pwords, w.pwords);
    expect("part_words", p.part_words, w.part_words);
    expect("fin_blocks", p.fin_blocks, w.fin_blocks);
    expect("hint_stride", p.hint_stride, w.hint_stride);
    expect("early", p.early, w.early);
    expect("too_large", p.too_large, w.too_large);
}

struct Row {
    const char *what;
    Ask ask;
    Want want;
};
// ask:  b, directions, {nq}, {nt}, swapped, radius, CUs, forced family, GENPC_NN_PATH, _R, _Q, _U, _WPS
// plan: family (0 VALU, 1 fp32 MFMA, 3 f16, 4 cell search), form (0 four waves, 1 three per SIMD, 2 2048-target tile, 3 wide),
//       r, q, unit, nl, slice_len, {qblocks}, {slices}, {block_begin}, {unit_begin}, {fin_begin}, blocks, units, pwords,
//       part_words, fin_blocks, hint_stride, early, too_large
static const Row kTable[] = {
    {"the headline step",
     {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, -1, 0, 0, 0, 0},
     {3, 3, 0, 4, 4, 1, 2048, {16, 16}, {8, 8}, {0, 128}, {0, 16}, {0, 256}, 256, 32, 2, 524288, 512, 32, 1, 0}},
    {"13 scans",
     {13, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, -1, 0, 0, 0, 0},
     {3, 1, 0, 4, 4, 1, 2048, {32, 32}, {8, 8}, {0, 3328}, {0, 416}, {0, 3328}, 6656, 832, 2, 6815744, 6656, 416, 0, 0}},
    {"1 x 10501 vs 10007, 256 CUs",
     {1, 2, {10501, 10007}, {10007, 10501}, 1, 0, 256, -1, -1, 0, 0, 0, 0},
     {3, 0, 0, 4, 4, 1, 896, {21, 20}, {12, 12}, {0, 252}, {0, 21}, {0, 165}, 492, 41, 2, 492192, 322, 21, 1, 0}},
    {"3 x 9001 vs 12003, 256 CUs",
     {3, 2, {9001, 12003}, {12003, 9001}, 1, 0, 256, -1, -1, 0, 0, 0, 0},
     {3, 3, 0, 4, 4, 1, 3072, {9, 12}, {4, 3}, {0, 108}, {0, 27}, {0, 423}, 216, 63, 2, 432078, 987, 62, 0, 0}},
    {"4 x 4099 vs 8209, 256 CUs",
     {4, 2, {4099, 8209}, {8209, 4099}, 1, 0, 256, -1, -1, 0, 0, 0, 0},
     {3, 3, 0, 4, 4, 1, 1408, {5, 9}, {6, 3}, {0, 120}, {0, 20}, {0, 260}, 228, 56, 2, 393768, 776, 49, 0, 0}},
    {"1 x 10501 vs 10007, 64 CUs",
     {1, 2, {10501, 10007}, {10007, 10501}, 1, 0, 64, -1, -1, 0, 0, 0, 0},
     {3, 3, 0, 4, 4, 1, 3584, {11, 10}, {3, 3}, {0, 33}, {0, 11}, {0, 165}, 63, 21, 2, 123048, 322, 21, 0, 0}},
    {"3 x 9001 vs 12003, 64 CUs",
     {3, 2, {9001, 12003}, {12003, 9001}, 1, 0, 64, -1, -1, 0, 0, 0, 0},
     {3, 1, 0, 4, 4, 1, 2432, {18, 24}, {5, 4}, {0, 270}, {0, 54}, {0, 423}, 558, 126, 2, 558102, 987, 62, 0, 0}},
    {"4 x 4099 vs 8209, 64 CUs",
     {4, 2, {4099, 8209}, {8209, 4099}, 1, 0, 64, -1, -1, 0, 0, 0, 0},
     {3, 2, 0, 4, 4, 1, 1664, {9, 17}, {5, 3}, {0, 180}, {0, 36}, {0, 260}, 384, 104, 2, 360976, 776, 49, 0, 0}},
    {"just below 6e6 pairs: fp32 MFMA",
     {1, 2, {1731, 1733}, {1733, 1731}, 1, 0, 256, -1, -1, 0, 0, 0, 0},
     {1, 0, 0, 1, 1, 0, 256, {14, 14}, {7, 7}, {0, 98}, {0, 14}, {0, 0}, 196, 28, 3, 72744, 0, 0, 0, 0}},
    {"just above",
     {1, 2, {1732, 1733}, {1733, 1732}, 1, 0, 256, -1, -1, 0, 0, 0, 0},
     {3, 0, 0, 2, 2, 1, 256, {7, 7}, {7, 7}, {0, 49}, {0, 7}, {0, 28}, 98, 14, 2, 48510, 56, 4, 1, 0}},
    {"below 6e6 pairs, f16 forced",
     {1, 2, {1731, 1733}, {1733, 1731}, 1, 0, 256, 3, -1, 0, 0, 0, 0},
     {3, 0, 0, 2, 2, 1, 256, {7, 7}, {7, 7}, {0, 49}, {0, 7}, {0, 28}, 98, 14, 2, 48496, 56, 4, 1, 0}},
    {"below 6e6 pairs, f16 by the switch",
     {1, 2, {1731, 1733}, {1733, 1731}, 1, 0, 256, -1, 3, 0, 0, 0, 0},
     {3, 0, 0, 2, 2, 1, 256, {7, 7}, {7, 7}, {0, 49}, {0, 7}, {0, 28}, 98, 14, 2, 48496, 56, 4, 1, 0}},
    {"1 x 1024^2",
     {1, 2, {1024, 1024}, {1024, 1024}, 1, 0, 256, -1, -1, 0, 0, 0, 0},
     {1, 0, 0, 1, 1, 0, 256, {8, 8}, {4, 4}, {0, 32}, {0, 8}, {0, 0}, 64, 16, 3, 24576, 0, 0, 0, 0}},
    {"a radius-limited call",
     {2, 2, {5000, 7000}, {7000, 5000}, 1, 1, 256, -1, -1, 0, 0, 0, 0},
     {4, 0, 0, 0, 0, 0, 0, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, 0, 0, 0, 0, 0, 0, 0, 0}},
    {"a radius-limited call, one direction",
     {2, 1, {5000, 0}, {7000, 0}, 0, 1, 256, -1, -1, 0, 0, 0, 0},
     {4, 0, 0, 0, 0, 0, 0, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, 0, 0, 0, 0, 0, 0, 0, 0}},
    {"cell search forced, directions that are no swaps: f16",
     {2, 2, {5000, 6000}, {7000, 8000}, 0, 0, 256, 4, -1, 0, 0, 0, 0},
     {3, 0, 0, 2, 2, 1, 896, {20, 24}, {8, 9}, {0, 320}, {0, 40}, {0, 158}, 752, 88, 2, 376000, 346, 22, 1, 0}},
    {"2^25 targets: fp32 MFMA",
     {1, 1, {1000, 0}, {33554432, 0}, 0, 0, 256, -1, -1, 0, 0, 0, 0},
     {1, 0, 0, 1, 2, 0, 262144, {8, 0}, {128, 0}, {0, 0}, {0, 0}, {0, 0}, 1024, 8, 3, 384000, 0, 0, 0, 0}},
    {"2^25 - 1 targets: f16",
     {1, 1, {1000, 0}, {33554431, 0}, 0, 0, 256, -1, -1, 0, 0, 0, 0},
     {3, 3, 0, 4, 4, 1, 2097152, {1, 0}, {16, 0}, {0, 0}, {0, 0}, {0, 0}, 16, 1, 2, 32000, 16, 1, 1, 0}},
    {"too large for one launch: the filter's blocks",
     {2000000, 1, {1000000, 0}, {1000, 0}, 0, 0, 256, -1, -1, 0, 0, 0, 0},
     {3, 1, 0, 4, 2, 2, 1024, {1954, 0}, {1, 0}, {0, 0}, {0, 0}, {0, 0}, 3908000000, 3908000000, 4, 8000000000000, 31250000000, 1953125000, 0, 1}},
    {"too large for one launch: the finish blocks alone",
     {100000, 1, {2000000, 0}, {100, 0}, 0, 0, 256, -1, -1, 0, 0, 0, 0},
     {3, 1, 0, 4, 2, 2, 128, {3907, 0}, {1, 0}, {0, 0}, {0, 0}, {0, 0}, 390700000, 390700000, 4, 800000000000, 3125000000, 195312500, 0, 1}},
    {"a radius, directions that are no swaps: f16 (the radius is not honoured)",
     {2, 2, {5000, 6000}, {7000, 8000}, 0, 1, 256, -1, -1, 0, 0, 0, 0},
     {3, 0, 0, 2, 2, 1, 896, {20, 24}, {8, 9}, {0, 320}, {0, 40}, {0, 158}, 752, 88, 2, 376000, 346, 22, 1, 0}},
    {"nothing to do",
     {1, 0, {0, 0}, {0, 0}, 0, 0, 256, -1, -1, 0, 0, 0, 0},
     {0, 0, 0, 0, 0, 0, 0, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, 0, 0, 0, 0, 0, 0, 0, 0}},
    {"GENPC_NN_R=0, VALU",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 0, -1, 0, 0, 0, 0},
     {0, 0, 2, 0, 0, 0, 256, {6, 10}, {20, 12}, {0, 240}, {0, 12}, {0, 0}, 480, 32, 1, 240000, 0, 0, 0, 0}},
    {"GENPC_NN_R=1, VALU",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 0, -1, 1, 0, 0, 0},
     {0, 0, 2, 0, 0, 0, 256, {6, 10}, {20, 12}, {0, 240}, {0, 12}, {0, 0}, 480, 32, 1, 240000, 0, 0, 0, 0}},
    {"GENPC_NN_R=2, VALU",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 0, -1, 2, 0, 0, 0},
     {0, 0, 2, 0, 0, 0, 256, {6, 10}, {20, 12}, {0, 240}, {0, 12}, {0, 0}, 480, 32, 1, 240000, 0, 0, 0, 0}},
    {"GENPC_NN_R=3, VALU",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 0, -1, 3, 0, 0, 0},
     {0, 0, 2, 0, 0, 0, 256, {6, 10}, {20, 12}, {0, 240}, {0, 12}, {0, 0}, 480, 32, 1, 240000, 0, 0, 0, 0}},
    {"GENPC_NN_R=4, VALU",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 0, -1, 4, 0, 0, 0},
     {0, 0, 4, 0, 0, 0, 256, {3, 5}, {20, 12}, {0, 120}, {0, 6}, {0, 0}, 240, 16, 1, 240000, 0, 0, 0, 0}},
    {"GENPC_NN_R=8, VALU",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 0, -1, 8, 0, 0, 0},
     {0, 0, 2, 0, 0, 0, 256, {6, 10}, {20, 12}, {0, 240}, {0, 12}, {0, 0}, 480, 32, 1, 240000, 0, 0, 0, 0}},
    {"GENPC_NN_R=-1, VALU",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 0, -1, -1, 0, 0, 0},
     {0, 0, 2, 0, 0, 0, 256, {6, 10}, {20, 12}, {0, 240}, {0, 12}, {0, 0}, 480, 32, 1, 240000, 0, 0, 0, 0}},
    {"GENPC_NN_Q=0, f16",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 0, 0, 0},
     {3, 0, 0, 2, 2, 1, 384, {12, 20}, {14, 8}, {0, 336}, {0, 24}, {0, 94}, 656, 64, 2, 328000, 252, 16, 1, 0}},
    {"GENPC_NN_Q=1, f16",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 1, 0, 0},
     {3, 0, 0, 2, 2, 1, 384, {12, 20}, {14, 8}, {0, 336}, {0, 24}, {0, 94}, 656, 64, 2, 328000, 252, 16, 1, 0}},
    {"GENPC_NN_Q=2, f16",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 2, 0, 0},
     {3, 0, 0, 2, 2, 1, 384, {12, 20}, {14, 8}, {0, 336}, {0, 24}, {0, 94}, 656, 64, 2, 328000, 252, 16, 1, 0}},
    {"GENPC_NN_Q=3, f16",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 3, 0, 0},
     {3, 0, 0, 2, 2, 1, 384, {12, 20}, {14, 8}, {0, 336}, {0, 24}, {0, 94}, 656, 64, 2, 328000, 252, 16, 1, 0}},
    {"GENPC_NN_Q=4, f16",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 4, 0, 0},
     {3, 0, 0, 4, 2, 1, 384, {6, 10}, {14, 8}, {0, 168}, {0, 12}, {0, 94}, 328, 32, 2, 328000, 252, 16, 1, 0}},
    {"GENPC_NN_Q=8, f16",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 8, 0, 0},
     {3, 0, 0, 2, 2, 1, 384, {12, 20}, {14, 8}, {0, 336}, {0, 24}, {0, 94}, 656, 64, 2, 328000, 252, 16, 1, 0}},
    {"GENPC_NN_Q=-1, f16",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, -1, 0, 0},
     {3, 0, 0, 2, 2, 1, 384, {12, 20}, {14, 8}, {0, 336}, {0, 24}, {0, 94}, 656, 64, 2, 328000, 252, 16, 1, 0}},
    {"GENPC_NN_Q=0, fp32 MFMA",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 0, 0, 0},
     {1, 0, 0, 1, 1, 0, 512, {24, 40}, {10, 6}, {0, 480}, {0, 48}, {0, 0}, 960, 128, 3, 360000, 0, 0, 0, 0}},
    {"GENPC_NN_Q=1, fp32 MFMA",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 1, 0, 0},
     {1, 0, 0, 1, 1, 0, 512, {24, 40}, {10, 6}, {0, 480}, {0, 48}, {0, 0}, 960, 128, 3, 360000, 0, 0, 0, 0}},
    {"GENPC_NN_Q=2, fp32 MFMA",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 2, 0, 0},
     {1, 0, 0, 2, 1, 0, 256, {12, 20}, {20, 12}, {0, 480}, {0, 24}, {0, 0}, 960, 64, 3, 720000, 0, 0, 0, 0}},
    {"GENPC_NN_Q=3, fp32 MFMA",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 3, 0, 0},
     {1, 0, 0, 1, 1, 0, 512, {24, 40}, {10, 6}, {0, 480}, {0, 48}, {0, 0}, 960, 128, 3, 360000, 0, 0, 0, 0}},
    {"GENPC_NN_Q=4, fp32 MFMA",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 4, 0, 0},
     {1, 0, 0, 1, 1, 0, 256, {6, 10}, {20, 12}, {0, 240}, {0, 12}, {0, 0}, 480, 32, 3, 720000, 0, 0, 0, 0}},
    {"GENPC_NN_Q=8, fp32 MFMA",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 8, 0, 0},
     {1, 0, 0, 1, 1, 0, 512, {24, 40}, {10, 6}, {0, 480}, {0, 48}, {0, 0}, 960, 128, 3, 360000, 0, 0, 0, 0}},
    {"GENPC_NN_Q=-1, fp32 MFMA",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, -1, 0, 0},
     {1, 0, 0, 1, 1, 0, 512, {24, 40}, {10, 6}, {0, 480}, {0, 48}, {0, 0}, 960, 128, 3, 360000, 0, 0, 0, 0}},
    {"GENPC_NN_U=0, f16",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 0, 0, 0},
     {3, 0, 0, 2, 2, 1, 384, {12, 20}, {14, 8}, {0, 336}, {0, 24}, {0, 94}, 656, 64, 2, 328000, 252, 16, 1, 0}},
    {"GENPC_NN_U=1, f16",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 0, 1, 0},
     {3, 0, 0, 2, 2, 1, 384, {12, 20}, {14, 8}, {0, 336}, {0, 24}, {0, 94}, 656, 64, 2, 328000, 252, 16, 1, 0}},
    {"GENPC_NN_U=2, f16",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 0, 2, 0},
     {3, 0, 0, 2, 2, 1, 384, {12, 20}, {14, 8}, {0, 336}, {0, 24}, {0, 94}, 656, 64, 2, 328000, 252, 16, 1, 0}},
    {"GENPC_NN_U=3, f16",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 0, 3, 0},
     {3, 0, 0, 2, 2, 1, 384, {12, 20}, {14, 8}, {0, 336}, {0, 24}, {0, 94}, 656, 64, 2, 328000, 252, 16, 1, 0}},
    {"GENPC_NN_U=4, f16",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 0, 4, 0},
     {3, 0, 0, 2, 4, 1, 384, {12, 20}, {14, 8}, {0, 336}, {0, 24}, {0, 94}, 656, 64, 2, 328000, 252, 16, 1, 0}},
    {"GENPC_NN_U=8, f16",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 0, 8, 0},
     {3, 0, 0, 2, 2, 1, 384, {12, 20}, {14, 8}, {0, 336}, {0, 24}, {0, 94}, 656, 64, 2, 328000, 252, 16, 1, 0}},
    {"GENPC_NN_U=-1, f16",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 0, -1, 0},
     {3, 0, 0, 2, 2, 1, 384, {12, 20}, {14, 8}, {0, 336}, {0, 24}, {0, 94}, 656, 64, 2, 328000, 252, 16, 1, 0}},
    {"GENPC_NN_U=0, fp32 MFMA",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 0, 0, 0},
     {1, 0, 0, 1, 1, 0, 512, {24, 40}, {10, 6}, {0, 480}, {0, 48}, {0, 0}, 960, 128, 3, 360000, 0, 0, 0, 0}},
    {"GENPC_NN_U=1, fp32 MFMA",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 0, 1, 0},
     {1, 0, 0, 1, 1, 0, 512, {24, 40}, {10, 6}, {0, 480}, {0, 48}, {0, 0}, 960, 128, 3, 360000, 0, 0, 0, 0}},
    {"GENPC_NN_U=2, fp32 MFMA",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 0, 2, 0},
     {1, 0, 0, 1, 2, 0, 512, {24, 40}, {10, 6}, {0, 480}, {0, 48}, {0, 0}, 960, 128, 3, 360000, 0, 0, 0, 0}},
    {"GENPC_NN_U=3, fp32 MFMA",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 0, 3, 0},
     {1, 0, 0, 1, 1, 0, 512, {24, 40}, {10, 6}, {0, 480}, {0, 48}, {0, 0}, 960, 128, 3, 360000, 0, 0, 0, 0}},
    {"GENPC_NN_U=4, fp32 MFMA",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 0, 4, 0},
     {1, 0, 0, 1, 1, 0, 512, {24, 40}, {10, 6}, {0, 480}, {0, 48}, {0, 0}, 960, 128, 3, 360000, 0, 0, 0, 0}},
    {"GENPC_NN_U=8, fp32 MFMA",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 0, 8, 0},
     {1, 0, 0, 1, 1, 0, 512, {24, 40}, {10, 6}, {0, 480}, {0, 48}, {0, 0}, 960, 128, 3, 360000, 0, 0, 0, 0}},
    {"GENPC_NN_U=-1, fp32 MFMA",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 0, -1, 0},
     {1, 0, 0, 1, 1, 0, 512, {24, 40}, {10, 6}, {0, 480}, {0, 48}, {0, 0}, 960, 128, 3, 360000, 0, 0, 0, 0}},
    {"GENPC_NN_WPS=0, the headline step",
     {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, -1, 0, 0, 0, 0},
     {3, 3, 0, 4, 4, 1, 2048, {16, 16}, {8, 8}, {0, 128}, {0, 16}, {0, 256}, 256, 32, 2, 524288, 512, 32, 1, 0}},
    {"GENPC_NN_WPS=1, the headline step",
     {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, -1, 0, 0, 0, 1},
     {3, 3, 0, 4, 4, 1, 4096, {16, 16}, {4, 4}, {0, 64}, {0, 16}, {0, 256}, 128, 32, 2, 262144, 512, 32, 1, 0}},
    {"GENPC_NN_WPS=2, the headline step",
     {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, -1, 0, 0, 0, 2},
     {3, 3, 0, 4, 4, 1, 2048, {16, 16}, {8, 8}, {0, 128}, {0, 16}, {0, 256}, 256, 32, 2, 524288, 512, 32, 1, 0}},
    {"GENPC_NN_WPS=3, the headline step",
     {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, -1, 0, 0, 0, 3},
     {3, 2, 0, 4, 4, 1, 1408, {32, 32}, {12, 12}, {0, 384}, {0, 32}, {0, 256}, 768, 64, 2, 786432, 512, 32, 1, 0}},
    {"GENPC_NN_WPS=8, the headline step",
     {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, -1, 0, 0, 0, 8},
     {3, 0, 0, 4, 4, 1, 1024, {32, 32}, {16, 16}, {0, 512}, {0, 32}, {0, 256}, 1024, 64, 2, 1048576, 512, 32, 1, 0}},
    {"GENPC_NN_WPS=-1, the headline step",
     {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, -1, 0, 0, 0, -1},
     {3, 3, 0, 4, 4, 1, 2048, {16, 16}, {8, 8}, {0, 128}, {0, 16}, {0, 256}, 256, 32, 2, 524288, 512, 32, 1, 0}},
    {"GENPC_NN_WPS=0, VALU",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 0, -1, 0, 0, 0, 0},
     {0, 0, 2, 0, 0, 0, 256, {6, 10}, {20, 12}, {0, 240}, {0, 12}, {0, 0}, 480, 32, 1, 240000, 0, 0, 0, 0}},
    {"GENPC_NN_WPS=1, VALU",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 0, -1, 0, 0, 0, 1},
     {0, 0, 2, 0, 0, 0, 480, {6, 10}, {11, 7}, {0, 132}, {0, 12}, {0, 0}, 272, 32, 1, 136000, 0, 0, 0, 0}},
    {"GENPC_NN_WPS=8, VALU",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 0, -1, 0, 0, 0, 8},
     {0, 0, 2, 0, 0, 0, 256, {6, 10}, {20, 12}, {0, 240}, {0, 12}, {0, 0}, 480, 32, 1, 240000, 0, 0, 0, 0}},
    {"GENPC_NN_WPS=-1, VALU",
     {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 0, -1, 0, 0, 0, -1},
     {0, 0, 2, 0, 0, 0, 256, {6, 10}, {20, 12}, {0, 240}, {0, 12}, {0, 0}, 480, 32, 1, 240000, 0, 0, 0, 0}},
    {"GENPC_NN_PATH -> -1",
     {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, -1, 0, 0, 0, 0},
     {3, 3, 0, 4, 4, 1, 2048, {16, 16}, {8, 8}, {0, 128}, {0, 16}, {0, 256}, 256, 32, 2, 524288, 512, 32, 1, 0}},
    {"GENPC_NN_PATH -> 0",
     {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, 0, 0, 0, 0, 0},
     {0, 0, 2, 0, 0, 0, 1024, {32, 32}, {16, 16}, {0, 512}, {0, 32}, {0, 0}, 1024, 64, 1, 524288, 0, 0, 0, 0}},
    {"GENPC_NN_PATH -> 1",
     {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, 1, 0, 0, 0, 0},
     {1, 0, 0, 1, 2, 0, 4096, {128, 128}, {4, 4}, {0, 512}, {0, 128}, {0, 0}, 1024, 256, 3, 393216, 0, 0, 0, 0}},
    {"GENPC_NN_PATH -> 3",
     {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, 3, 0, 0, 0, 0},
     {3, 3, 0, 4, 4, 1, 2048, {16, 16}, {8, 8}, {0, 128}, {0, 16}, {0, 256}, 256, 32, 2, 524288, 512, 32, 1, 0}},
    {"GENPC_NN_PATH -> 4",
     {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, 4, 0, 0, 0, 0},
     {4, 0, 0, 0, 0, 0, 0, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, 0, 0, 0, 0, 0, 0, 0, 0}},
    {"GENPC_NN_PATH -> 2",
     {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, 2, 0, 0, 0, 0},
     {3, 3, 0, 4, 4, 1, 2048, {16, 16}, {8, 8}, {0, 128}, {0, 16}, {0, 256}, 256, 32, 2, 524288, 512, 32, 1, 0}},
    {"GENPC_NN_PATH -> 7",
     {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, 7, 0, 0, 0, 0},
     {3, 3, 0, 4, 4, 1, 2048, {16, 16}, {8, 8}, {0, 128}, {0, 16}, {0, 256}, 256, 32, 2, 524288, 512, 32, 1, 0}},
};

static void table()
{
    for (const Row &r : kTable) row(r.what, r.ask, r.want);
}

static void fail(const NNAsk &a, const char *what, long long v)
{
    if (g_failed++ < 30)
        printf("FAILED %s (%lld): b %d, %d direction(s) %d x %d / %d x %d, %d CUs, family forced %d\n", what, v, a.b, a.ndir, a.nq[0], a.nt[0], a.nq[1], a.nt[1], a.cus,
               a.forced);
}

// what must hold for every plan, whatever the thresholds are
static void properties()
{
    const int sizes[] = {1, 15, 16, 17, 37, 127, 128, 513, 1000, 1024, 2047, 2049, 4099, 8192, 8209, 10007, 12003, 16384, 20011, 32771, 65537, 165546};
    long long seen[4] = {0, 0, 0, 0};
    for (int b : {1, 2, 3, 4, 5, 7, 8, 13, 16, 1000})
        for (int n : sizes)
            for (int m : sizes)
                for (int nd = 1; nd <= 2; nd++)
                    for (int cus : {32, 64, 128, 256, 304})
                        for (int forced : {-1, 0, 1, 3}) {
                            NNAsk a;
                            a.b = b;
                            a.cus = cus;
                            a.forced = forced;
                            a.add(n, m);
                            if (nd == 2) a.add(m, n);
                            a.swapped = nd == 2;
                            const NNPlan p = nn_plan(a);
                            if (p.too_large) fail(a, "too large", p.blocks);
                            const bool f16 = p.family == kNNF16;
                            const int gran = f16 ? 128 : (p.family == kNNMfma32 ? 64 : 32);
                            if (p.slice_len <= 0 || p.slice_len % gran) fail(a, "slice_len is no multiple of the family's granularity", p.slice_len);
                            // queries per block
                            const int qper = p.family == kNNValu ? 256 * p.r : 128 * p.q * (f16 && p.form == kNNWide ? 2 : 1);
                            if (p.family == kNNValu ? (p.r != 2 && p.r != 4) : (f16 ? (p.q != 2 && p.q != 4) : (p.q != 1 && p.q != 2))) fail(a, "q / r", p.q);
                            if (f16 ? (p.unit != 2 && p.unit != 4) : (p.family == kNNMfma32 && p.unit != 1 && p.unit != 2)) fail(a, "unit", p.unit);
                            long long blocks = 0, units = 0, fin = 0, four_wave_blocks = 0;
                            for (int d = 0; d < nd; d++) {
                                const NNPlanDir &D = p.dir[d];
                                if ((long long)D.qblocks * qper < a.nq[d] || (long long)(D.qblocks - 1) * qper >= a.nq[d]) fail(a, "qblocks do not cover the queries", D.qblocks);
                                if ((long long)D.slices * p.slice_len < a.nt[d] || (long long)(D.slices - 1) * p.slice_len >= a.nt[d]) fail(a, "slices do not cover the targets", D.slices);
                                if (f16 && D.slices * p.nl > kMaxLists) fail(a, "more lists than kMaxLists", D.slices * p.nl);
                                // the directions' ranges of blocks, counters and finish blocks follow each other
                                if (D.block_begin != blocks || D.unit_begin != units || D.fin_begin != fin) fail(a, "ranges of the directions overlap or leave a gap", d);
                                blocks += (long long)D.slices * b * D.qblocks;
                                units += (long long)b * D.qblocks;
                                if (f16) fin += (long long)b * ((a.nq[d] + 63) / 64);
                                four_wave_blocks += (long long)D.slices * b * ((a.nq[d] + 511) / 512);
                                if (D.partials != (f16 || D.slices > 1)) fail(a, "partials", d);
                            }
                            if (blocks != p.blocks || units != p.units || fin != p.fin_blocks) fail(a, "totals", blocks);
                            if (!f16) continue;
                            if (p.nl != 1 && p.nl != 2) fail(a, "nl", p.nl);
                            if (p.pwords != 2 * p.nl) fail(a, "pwords", p.pwords);
                            if (p.q == 2 && p.form != kNNFourWave) fail(a, "a form of the 512-query blocks with Q = 2", p.form);
                            // wide: one round -- the four-wave blocks of the same slices would all be resident, two per CU
                            if (p.form == kNNWide && (four_wave_blocks > 2LL * cus || p.slice_len <= 1024)) fail(a, "wide form outside a single round", four_wave_blocks);
                            if (p.form == kNNTile2048 && p.slice_len <= 1024) fail(a, "2048-target tile for a short slice", p.slice_len);
                            // three waves per SIMD: three blocks per CU resident, at least three rounds of them
                            if (p.form == kNNThreeWave && p.blocks <= 2LL * 3 * cus) fail(a, "three-wave form with fewer than three rounds", p.blocks);
                            if (p.early != (p.fin_blocks <= 2LL * cus)) fail(a, "early", p.early);
                            if ((long long)p.hint_stride * 16 < p.fin_blocks) fail(a, "more than 16 reports", p.hint_stride);
                            seen[p.form]++;
                        }
    for (int f = 0; f < 4; f++)
        if (!seen[f]) { printf("FAILED: the sweep never met form %d\n", f); g_failed++; }
}

int main(int argc, char **argv)
{
    g_print = argc > 1 && !strcmp(argv[1], "--exported");
    table();
    if (g_print) return 0;
    // a direction without queries or targets is no part of the ask
    NNAsk a;
    a.b = 2;
    if (a.add(0, 5) || a.add(5, 0) || a.add(-1, 5) || !a.add(5, 7) || a.ndir != 1 || a.nq[0] != 5 || a.nt[0] != 7) { printf("FAILED: NNAsk::add\n"); g_failed++; }
    NNAsk z;
    if (z.add(5, 7) || z.ndir != 0) { printf("FAILED: NNAsk::add with b = 0\n"); g_failed++; }
    properties();
    if (g_failed) {
        printf("nn_plan_check: %d check(s) failed\n", g_failed);
        return 1;
    }
    printf("nn_plan_check: ok\n");
    return 0;
}
