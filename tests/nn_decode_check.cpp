// Stand-alone check of genpc_amd/csrc/nn_decode.h (plain C++; tests/test_nn_entry_args.py builds it with
// -fsanitize=address,undefined and runs it).  Exit status 0 = every check passed; each failure prints what it found.
//  1. nn_div against / for every divisor from 1 to 4096 and a list of large ones, each over every block id up to 2^20 and the
//     ids just below and just above every multiple of the divisor near 2^31 - 1;
//  2. the full decode of a filter block and of a finish block, against / and %, for every block of the plans that nn_plan gives
//     for EVERY ask of tests/nn_plan_check.cpp's table (repeated here as literals, label by label -- the test compares the two
//     files; the plans come from the header) and for three asks of its own.  Rows that launch none of the four kernels (cell
//     search, nothing to do, too large) have nothing to decode and are counted.
#include "nn_decode.h"

#include <stdio.h>

using namespace genpc;

static int g_failed = 0;

static void fail(const char *what, long long d, long long n, long long got, long long want)
{
    if (g_failed < 20) printf("FAILED %s: divisor %lld, id %lld: %lld, expected %lld\n", what, d, n, got, want);
    g_failed++;
}

static void check_div(int d)
{
    const NNDiv v = nn_div_make(d);
    if (v.shift > 31) fail("shift", d, 0, v.shift, 31);
    auto one = [&](long long n) {
        if (n < 0 || n > 0x7fffffffLL) return;
        const int q = nn_div((int)n, v);
        if (q != (int)(n / d)) fail("nn_div", d, n, q, n / d);
        if (nn_is_multiple((int)n, d, v) != (n % d == 0)) fail("nn_is_multiple", d, n, nn_is_multiple((int)n, d, v), n % d == 0);
    };
    for (long long n = 0; n <= (1 << 20); n++) one(n);
    // multiples of d near 2^31 - 1: the last sixteen of them (and what would be the next), one id below, the id, one above
    const long long top = 0x7fffffffLL / d;
    for (long long k = top - 15; k <= top + 1; k++) {
        if (k < 0) continue;
        for (long long e = -2; e <= 2; e++) one(k * d + e);
    }
    one(0x7fffffffLL);
    one(0x7ffffffeLL);
}

struct Ask {
    int b, ndir, nq[2], nt[2], swapped, radius, cus, forced, env_family, env_r, env_q, env_u, env_wps;
};
struct Case {
    const char *what;
    Ask ask;
};
// b, directions, {nq}, {nt}, swapped, radius, CUs, forced family, GENPC_NN_PATH, _R, _Q, _U, _WPS
// EVERY row of nn_plan_check.cpp's table, label and ask as they stand there, in its order (tests/test_nn_entry_args.py compares
// the two lists as text).  The rows whose plan is the cell search, nothing to do or too large launch none of the four kernels:
// check_plan() counts them and main() says how many of each there were.
static const Case kTableAsks[] = {
    {"the headline step", {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, -1, 0, 0, 0, 0}},
    {"13 scans", {13, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, -1, 0, 0, 0, 0}},
    {"1 x 10501 vs 10007, 256 CUs", {1, 2, {10501, 10007}, {10007, 10501}, 1, 0, 256, -1, -1, 0, 0, 0, 0}},
    {"3 x 9001 vs 12003, 256 CUs", {3, 2, {9001, 12003}, {12003, 9001}, 1, 0, 256, -1, -1, 0, 0, 0, 0}},
    {"4 x 4099 vs 8209, 256 CUs", {4, 2, {4099, 8209}, {8209, 4099}, 1, 0, 256, -1, -1, 0, 0, 0, 0}},
    {"1 x 10501 vs 10007, 64 CUs", {1, 2, {10501, 10007}, {10007, 10501}, 1, 0, 64, -1, -1, 0, 0, 0, 0}},
    {"3 x 9001 vs 12003, 64 CUs", {3, 2, {9001, 12003}, {12003, 9001}, 1, 0, 64, -1, -1, 0, 0, 0, 0}},
    {"4 x 4099 vs 8209, 64 CUs", {4, 2, {4099, 8209}, {8209, 4099}, 1, 0, 64, -1, -1, 0, 0, 0, 0}},
    {"just below 6e6 pairs: fp32 MFMA", {1, 2, {1731, 1733}, {1733, 1731}, 1, 0, 256, -1, -1, 0, 0, 0, 0}},
    {"just above", {1, 2, {1732, 1733}, {1733, 1732}, 1, 0, 256, -1, -1, 0, 0, 0, 0}},
    {"below 6e6 pairs, f16 forced", {1, 2, {1731, 1733}, {1733, 1731}, 1, 0, 256, 3, -1, 0, 0, 0, 0}},
    {"below 6e6 pairs, f16 by the switch", {1, 2, {1731, 1733}, {1733, 1731}, 1, 0, 256, -1, 3, 0, 0, 0, 0}},
    {"1 x 1024^2", {1, 2, {1024, 1024}, {1024, 1024}, 1, 0, 256, -1, -1, 0, 0, 0, 0}},
    {"a radius-limited call", {2, 2, {5000, 7000}, {7000, 5000}, 1, 1, 256, -1, -1, 0, 0, 0, 0}},
    {"a radius-limited call, one direction", {2, 1, {5000, 0}, {7000, 0}, 0, 1, 256, -1, -1, 0, 0, 0, 0}},
    {"cell search forced, directions that are no swaps: f16", {2, 2, {5000, 6000}, {7000, 8000}, 0, 0, 256, 4, -1, 0, 0, 0, 0}},
    {"2^25 targets: fp32 MFMA", {1, 1, {1000, 0}, {33554432, 0}, 0, 0, 256, -1, -1, 0, 0, 0, 0}},
    {"2^25 - 1 targets: f16", {1, 1, {1000, 0}, {33554431, 0}, 0, 0, 256, -1, -1, 0, 0, 0, 0}},
    {"too large for one launch: the filter's blocks", {2000000, 1, {1000000, 0}, {1000, 0}, 0, 0, 256, -1, -1, 0, 0, 0, 0}},
    {"too large for one launch: the finish blocks alone", {100000, 1, {2000000, 0}, {100, 0}, 0, 0, 256, -1, -1, 0, 0, 0, 0}},
    {"a radius, directions that are no swaps: f16 (the radius is not honoured)", {2, 2, {5000, 6000}, {7000, 8000}, 0, 1, 256, -1, -1, 0, 0, 0, 0}},
    {"nothing to do", {1, 0, {0, 0}, {0, 0}, 0, 0, 256, -1, -1, 0, 0, 0, 0}},
    {"GENPC_NN_R=0, VALU", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 0, -1, 0, 0, 0, 0}},
    {"GENPC_NN_R=1, VALU", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 0, -1, 1, 0, 0, 0}},
    {"GENPC_NN_R=2, VALU", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 0, -1, 2, 0, 0, 0}},
    {"GENPC_NN_R=3, VALU", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 0, -1, 3, 0, 0, 0}},
    {"GENPC_NN_R=4, VALU", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 0, -1, 4, 0, 0, 0}},
    {"GENPC_NN_R=8, VALU", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 0, -1, 8, 0, 0, 0}},
    {"GENPC_NN_R=-1, VALU", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 0, -1, -1, 0, 0, 0}},
    {"GENPC_NN_Q=0, f16", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 0, 0, 0}},
    {"GENPC_NN_Q=1, f16", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 1, 0, 0}},
    {"GENPC_NN_Q=2, f16", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 2, 0, 0}},
    {"GENPC_NN_Q=3, f16", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 3, 0, 0}},
    {"GENPC_NN_Q=4, f16", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 4, 0, 0}},
    {"GENPC_NN_Q=8, f16", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 8, 0, 0}},
    {"GENPC_NN_Q=-1, f16", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, -1, 0, 0}},
    {"GENPC_NN_Q=0, fp32 MFMA", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 0, 0, 0}},
    {"GENPC_NN_Q=1, fp32 MFMA", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 1, 0, 0}},
    {"GENPC_NN_Q=2, fp32 MFMA", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 2, 0, 0}},
    {"GENPC_NN_Q=3, fp32 MFMA", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 3, 0, 0}},
    {"GENPC_NN_Q=4, fp32 MFMA", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 4, 0, 0}},
    {"GENPC_NN_Q=8, fp32 MFMA", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 8, 0, 0}},
    {"GENPC_NN_Q=-1, fp32 MFMA", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, -1, 0, 0}},
    {"GENPC_NN_U=0, f16", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 0, 0, 0}},
    {"GENPC_NN_U=1, f16", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 0, 1, 0}},
    {"GENPC_NN_U=2, f16", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 0, 2, 0}},
    {"GENPC_NN_U=3, f16", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 0, 3, 0}},
    {"GENPC_NN_U=4, f16", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 0, 4, 0}},
    {"GENPC_NN_U=8, f16", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 0, 8, 0}},
    {"GENPC_NN_U=-1, f16", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 3, -1, 0, 0, -1, 0}},
    {"GENPC_NN_U=0, fp32 MFMA", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 0, 0, 0}},
    {"GENPC_NN_U=1, fp32 MFMA", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 0, 1, 0}},
    {"GENPC_NN_U=2, fp32 MFMA", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 0, 2, 0}},
    {"GENPC_NN_U=3, fp32 MFMA", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 0, 3, 0}},
    {"GENPC_NN_U=4, fp32 MFMA", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 0, 4, 0}},
    {"GENPC_NN_U=8, fp32 MFMA", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 0, 8, 0}},
    {"GENPC_NN_U=-1, fp32 MFMA", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 1, -1, 0, 0, -1, 0}},
    {"GENPC_NN_WPS=0, the headline step", {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, -1, 0, 0, 0, 0}},
    {"GENPC_NN_WPS=1, the headline step", {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, -1, 0, 0, 0, 1}},
    {"GENPC_NN_WPS=2, the headline step", {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, -1, 0, 0, 0, 2}},
    {"GENPC_NN_WPS=3, the headline step", {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, -1, 0, 0, 0, 3}},
    {"GENPC_NN_WPS=8, the headline step", {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, -1, 0, 0, 0, 8}},
    {"GENPC_NN_WPS=-1, the headline step", {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, -1, 0, 0, 0, -1}},
    {"GENPC_NN_WPS=0, VALU", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 0, -1, 0, 0, 0, 0}},
    {"GENPC_NN_WPS=1, VALU", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 0, -1, 0, 0, 0, 1}},
    {"GENPC_NN_WPS=8, VALU", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 0, -1, 0, 0, 0, 8}},
    {"GENPC_NN_WPS=-1, VALU", {2, 2, {3000, 5000}, {5000, 3000}, 1, 0, 256, 0, -1, 0, 0, 0, -1}},
    {"GENPC_NN_PATH -> -1", {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, -1, 0, 0, 0, 0}},
    {"GENPC_NN_PATH -> 0", {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, 0, 0, 0, 0, 0}},
    {"GENPC_NN_PATH -> 1", {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, 1, 0, 0, 0, 0}},
    {"GENPC_NN_PATH -> 3", {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, 3, 0, 0, 0, 0}},
    {"GENPC_NN_PATH -> 4", {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, 4, 0, 0, 0, 0}},
    {"GENPC_NN_PATH -> 2", {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, 2, 0, 0, 0, 0}},
    {"GENPC_NN_PATH -> 7", {1, 2, {16384, 16384}, {16384, 16384}, 1, 0, 256, -1, 7, 0, 0, 0, 0}},
};
// further asks, not in that table: the shapes of tests/test_gpu_nn_entry_args.py and a launch of 1000 batch elements
static const Case kOwnAsks[] = {
    {"7 x 700 vs 1300, f16", {7, 2, {700, 1300}, {1300, 700}, 1, 0, 256, 3, -1, 0, 0, 0, 0}},
    {"3 x 1300 vs 37, one direction, f16", {3, 1, {1300, 0}, {37, 0}, 0, 0, 256, 3, -1, 0, 0, 0, 0}},
    {"1000 x 4096 vs 777, 304 CUs", {1000, 2, {4096, 777}, {777, 4096}, 1, 0, 304, -1, -1, 0, 0, 0, 0}},
};

static int g_decoded = 0, g_grid = 0, g_nothing = 0, g_too_large = 0;

static void check_plan(const Case &c)
{
    const Ask &k = c.ask;
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
    const NNPlan p = nn_plan(a);
    if (a.ndir == 0) { g_nothing++; return; }
    if (p.family == kNNGrid) { g_grid++; return; }
    if (p.too_large) { g_too_large++; return; }
    g_decoded++;
    const NNDiv by_b = nn_div_make(a.b), by_hint = nn_div_make(p.hint_stride);
    for (int d = 0; d < a.ndir; d++) {
        // the first launch: block id within the direction = (slice * b + batch) * qblocks + qb
        const NNPlanDir &D = p.dir[d];
        const NNDiv by_q = nn_div_make(D.qblocks);
        const long long n = (long long)D.slices * a.b * D.qblocks;
        const long long end = d + 1 < a.ndir ? p.dir[d + 1].block_begin : p.blocks;
        if (D.block_begin + n != end) fail("blocks of the direction", d, D.block_begin, n, end - D.block_begin);
        for (long long bid = 0; bid < n; bid++) {
            const NNBlockId id = nn_decode_block((int)bid, D.qblocks, by_q, a.b, by_b);
            const long long rest = bid / D.qblocks;
            if (id.qb != bid % D.qblocks) fail("qb", D.qblocks, bid, id.qb, bid % D.qblocks);
            if (id.batch != rest % a.b) fail("batch", a.b, bid, id.batch, rest % a.b);
            if (id.slice != rest / a.b) fail("slice", a.b, bid, id.slice, rest / a.b);
        }
        if (p.family != kNNF16) continue;
        // the finish launch: block id within the direction = batch * fblocks + fb
        const int fblocks = nn_fin_blocks(a.nq[d]);
        const NNDiv by_f = nn_div_make(fblocks);
        const long long fn = (long long)a.b * fblocks;
        const long long fend = d + 1 < a.ndir ? p.dir[d + 1].fin_begin : p.fin_blocks;
        if (D.fin_begin + fn != fend) fail("finish blocks of the direction", d, D.fin_begin, fn, fend - D.fin_begin);
        for (long long bid = 0; bid < fn; bid++) {
            const NNFinId id = nn_decode_fin((int)bid, fblocks, by_f);
            if (id.batch != bid / fblocks) fail("finish batch", fblocks, bid, id.batch, bid / fblocks);
            if (id.fb != bid % fblocks) fail("fb", fblocks, bid, id.fb, bid % fblocks);
            const long long g = D.fin_begin + bid;      // the report is sampled over the launch's block ids
            if (nn_is_multiple((int)g, p.hint_stride, by_hint) != (g % p.hint_stride == 0)) fail("hint", p.hint_stride, g, 0, 0);
        }
    }
}

int main()
{
    for (int d = 1; d <= 4096; d++) check_div(d);
    // large divisors: 13 x 416 (the 13 scans' query blocks), 2^31 - 1, primes near 2^16 and 2^20, powers of two and their neighbours
    const int large[] = {13 * 416, 0x7fffffff, 0x7ffffffe, 0x40000000, 0x40000001, 0x3fffffff, 65521, 65537, 65539, 1048573, 1048583,
                         1048576, 1048577, 65536, 65535, 6656, 3328, 195312500, 1953125000, 100000, 1000003, 16777259};
    for (int d : large) check_div(d);
    for (const Case &c : kTableAsks) check_plan(c);
    const int table_rows = (int)(sizeof(kTableAsks) / sizeof(kTableAsks[0]));
    printf("nn_decode_check: %d rows of the plan table: %d decoded block by block, %d cell search, %d nothing to do, %d too large\n", table_rows, g_decoded,
           g_grid, g_nothing, g_too_large);
    if (g_decoded + g_grid + g_nothing + g_too_large != table_rows) {
        printf("FAILED: rows of the table that were not decoded\n");
        g_failed++;
    }
    for (const Case &c : kOwnAsks) check_plan(c);
    if (g_failed) {
        printf("nn_decode_check: %d FAILED\n", g_failed);
        return 1;
    }
    printf("nn_decode_check: ok\n");
    return 0;
}
