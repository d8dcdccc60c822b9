// Stand-alone check of genpc_amd/csrc/hpr_plan.h (host code only; tests/test_hpr_plan.py builds it with
// -fsanitize=address,undefined and runs it).  Exit status 0 = every check passed; each failure prints what it found.
// The table holds asks and the plans they must give as literals -- worked by hand from hpr_run as it stood before the plan was
// taken out of it, no second copy of the header's expressions; the properties below it are checked over a sweep of shapes, CU
// counts and switches.
// `hpr_plan_check --exported` prints, for the rows that genpc_hpr_plan can be asked (no switch set), "c n best_only cus : the
// twenty-four values of out[]" from the table's literals.
#include "hpr_plan.h"

#include <stdio.h>
#include <string.h>

using namespace genpc;

static int g_failed = 0;
static bool g_print = false;

struct Ask {
    int c, n, best_only, cus, env_split, env_park_mb, env_home_tiles, env_home_chunks, env_decide_kernel, no_cull;
};
struct Want {
    int too_large, ntiles, split, prune, key_bits, max_clips, home_tiles, home_chunks;
    long long park_cap;
    int decide_kernel, row_grid, bounds_grid, view_grid, decide_blocks, walk_blocks, large_blocks, global_blocks, gcap;
};

static HprAsk ask_of(const Ask &k)
{
    HprAsk a;
    a.c = k.c;
    a.n = k.n;
    a.best_only = k.best_only;
    a.cus = k.cus;
    a.env_split = k.env_split;
    a.env_park_mb = k.env_park_mb;
    a.env_home_tiles = k.env_home_tiles;
    a.env_home_chunks = k.env_home_chunks;
    a.env_decide_kernel = k.env_decide_kernel;
    a.no_cull = k.no_cull;
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
        if (k.env_split != -1 || k.env_park_mb != 3072 || k.env_home_tiles != 1 || k.env_home_chunks != 2 || k.env_decide_kernel != 1 || k.no_cull) return;
        // (what the rows do not spell out is the same for every plan: 32 candidates marked at a time, the hand-over from batch 4
        // with at most 128 lanes left; the stores' sizes follow from park_cap, global_blocks and gcap)
        const int z = w.too_large;
        printf("%d %d %d %d : %d %d %d %d %d %d %d %d %d %d %d %lld %d %d %d %d %d %d %d %d %d %lld %lld %d\n", k.c, k.n, k.best_only, k.cus, w.too_large, w.ntiles,
               w.split, w.prune, w.key_bits, w.max_clips, w.home_tiles, w.home_chunks, z ? 0 : 32, z ? 0 : 4, z ? 0 : 128, w.park_cap, w.decide_kernel, w.row_grid,
               w.bounds_grid, w.view_grid, w.decide_blocks, w.walk_blocks, w.large_blocks, w.global_blocks, w.gcap, (w.park_cap * 160) >> 20,
               ((long long)w.global_blocks * 2 * w.gcap * 16) >> 20, k.cus);
        return;
    }
    const HprPlan p = hpr_plan(ask_of(k));
    expect("too_large", p.too_large, w.too_large);
    expect("ntiles", p.ntiles, w.ntiles);
    expect("split", p.split, w.split);
    expect("prune", p.prune, w.prune);
    expect("key_bits", p.key_bits, w.key_bits);
    expect("max_clips", p.max_clips, w.max_clips);
    expect("home_tiles", p.home_tiles, w.home_tiles);
    expect("home_chunks", p.home_chunks, w.home_chunks);
    expect("park_cap", p.park_cap, w.park_cap);
    expect("park_bytes", p.park_bytes, w.park_cap * 160);
    expect("decide_kernel", p.decide_kernel, w.decide_kernel);
    expect("row_grid", p.row_grid, w.row_grid);
    expect("bounds_grid", p.bounds_grid, w.bounds_grid);
    expect("view_grid", p.view_grid, w.view_grid);
    expect("decide_blocks", p.decide_blocks, w.decide_blocks);
    expect("walk_blocks", p.walk_blocks, w.walk_blocks);
    expect("large_blocks", p.large_blocks, w.large_blocks);
    expect("global_blocks", p.global_blocks, w.global_blocks);
    expect("gcap", p.gcap, w.gcap);
    expect("global_bytes", p.global_bytes, (long long)w.global_blocks * 2 * w.gcap * 16);
    if (w.too_large) return;
    expect("chunk_w", p.chunk_w, 32);
    expect("straggle_from", p.straggle_from, 4);
    expect("straggle_lanes", p.straggle_lanes, 128);
    expect("pairs", p.pairs, (long long)k.c * k.n);
    expect("fl_count", p.fl_count, 3ll * k.c * k.n);
    expect("tile_count", p.tile_count, (long long)k.c * w.ntiles);
    expect("surv_count", p.surv_count, w.split ? (long long)k.c * k.n : 0);
}

struct Row {
    const char *what;
    Ask ask;
    Want want;
};
// ask:  views, points, best_only, CUs, GENPC_HPR_SPLIT, _PARK_MB, _HOME_TILES, _HOME_CHUNKS, _DECIDE_KERNEL, _NOCULL
// plan: too_large, ntiles, split, prune, key_bits, max_clips, home_tiles, home_chunks, park_cap, decide_kernel, row_grid, bounds_grid,
//       view_grid, decide_blocks, walk_blocks, large_blocks, global_blocks, gcap
static const Row kTable[] = {
    {"viewpoint_select's shape", {64, 10000, 0, 256, -1, 3072, 1, 2, 1, 0}, {0, 79, 1, 0, 26, 256, 1, 2, 640000, 1, 40, 40, 1, 16384, 10240, 1280, 838, 10008}},
    {"two-kernel form at its threshold", {8, 12500, 0, 256, -1, 3072, 1, 2, 1, 0}, {0, 98, 1, 0, 23, 256, 1, 2, 100000, 1, 49, 49, 1, 16384, 10240, 1280, 670, 12508}},
    {"one pair below it", {8, 12499, 0, 256, -1, 3072, 1, 2, 1, 0}, {0, 98, 0, 0, 23, 256, 3, 4, 0, 0, 49, 49, 1, 16384, 10240, 1280, 670, 12507}},
    {"255 tiles", {4, 32640, 0, 256, -1, 3072, 1, 2, 1, 0}, {0, 255, 1, 0, 22, 256, 1, 2, 130560, 1, 128, 128, 1, 16384, 10240, 1280, 256, 32648}},
    {"256 tiles: the large-cloud form", {4, 32641, 0, 256, -1, 3072, 1, 2, 1, 0}, {0, 256, 0, 0, 22, 48, 3, 4, 0, 0, 128, 128, 1, 16384, 10240, 1280, 256, 32649}},
    {"the benchmark's large cloud", {2, 165546, 0, 256, -1, 3072, 1, 2, 1, 0}, {0, 1294, 0, 0, 21, 48, 3, 4, 0, 0, 647, 647, 1, 16384, 10240, 1280, 50, 165554}},
    {"GENPC_HPR_SPLIT=1, GENPC_HPR_PARK_MB=1: 160-byte polygons", {4, 3001, 0, 256, 1, 1, 1, 2, 1, 0}, {0, 24, 1, 0, 22, 256, 1, 2, 6553, 1, 12, 12, 1, 12008, 10240, 1280, 1024, 3009}},
    {"GENPC_HPR_PARK_MB=0 counts as 1", {4, 3001, 0, 256, 1, 0, 1, 2, 1, 0}, {0, 24, 1, 0, 22, 256, 1, 2, 6553, 1, 12, 12, 1, 12008, 10240, 1280, 1024, 3009}},
    {"GENPC_HPR_PARK_MB=-5 counts as 1", {4, 3001, 0, 256, 1, -5, 1, 2, 1, 0}, {0, 24, 1, 0, 22, 256, 1, 2, 6553, 1, 12, 12, 1, 12008, 10240, 1280, 1024, 3009}},
    {"one point", {1, 1, 0, 256, -1, 3072, 1, 2, 1, 0}, {0, 1, 0, 0, 20, 256, 3, 4, 0, 0, 1, 1, 1, 8, 1, 1, 1, 9}},
    {"three views of a small cloud: one kernel, three home tiles", {3, 3001, 0, 256, -1, 3072, 1, 2, 1, 0}, {0, 24, 0, 0, 22, 256, 3, 4, 0, 0, 12, 12, 1, 9008, 9003, 1280, 1024, 3009}},
    {"2 x 32641: the smallest large-cloud form", {2, 32641, 0, 256, -1, 3072, 1, 2, 1, 0}, {0, 256, 0, 0, 21, 48, 3, 4, 0, 0, 128, 128, 1, 16384, 10240, 1280, 256, 32649}},
    {"viewpoint_select's shape on 64 CUs", {64, 10000, 0, 64, -1, 3072, 1, 2, 1, 0}, {0, 79, 1, 0, 26, 256, 1, 2, 640000, 1, 40, 40, 1, 4096, 2560, 320, 838, 10008}},
    {"best view, two-kernel form: views are pruned", {64, 10000, 1, 256, -1, 3072, 1, 2, 1, 0}, {0, 79, 1, 1, 26, 256, 1, 2, 640000, 1, 40, 40, 1, 16384, 10240, 1280, 838, 10008}},
    {"best view, large cloud: not pruned", {2, 165546, 1, 256, -1, 3072, 1, 2, 1, 0}, {0, 1294, 0, 0, 21, 48, 3, 4, 0, 0, 647, 647, 1, 16384, 10240, 1280, 50, 165554}},
    {"best view, GENPC_HPR_SPLIT=0: not pruned", {64, 10000, 1, 256, 0, 3072, 1, 2, 1, 0}, {0, 79, 0, 0, 26, 256, 3, 4, 0, 0, 40, 40, 1, 16384, 10240, 1280, 838, 10008}},
    {"GENPC_HPR_HOME_TILES=0 -> 1", {64, 10000, 0, 256, -1, 3072, 0, 2, 1, 0}, {0, 79, 1, 0, 26, 256, 1, 2, 640000, 1, 40, 40, 1, 16384, 10240, 1280, 838, 10008}},
    {"GENPC_HPR_HOME_TILES=2: the chunks switch is ignored", {64, 10000, 0, 256, -1, 3072, 2, 1, 1, 0}, {0, 79, 1, 0, 26, 256, 2, 4, 640000, 1, 40, 40, 1, 16384, 10240, 1280, 838, 10008}},
    {"GENPC_HPR_HOME_TILES=3", {64, 10000, 0, 256, -1, 3072, 3, 2, 1, 0}, {0, 79, 1, 0, 26, 256, 3, 4, 640000, 1, 40, 40, 1, 16384, 10240, 1280, 838, 10008}},
    {"GENPC_HPR_HOME_TILES=7 -> 3", {64, 10000, 0, 256, -1, 3072, 7, 2, 1, 0}, {0, 79, 1, 0, 26, 256, 3, 4, 640000, 1, 40, 40, 1, 16384, 10240, 1280, 838, 10008}},
    {"GENPC_HPR_HOME_CHUNKS=0 -> 1", {64, 10000, 0, 256, -1, 3072, 1, 0, 1, 0}, {0, 79, 1, 0, 26, 256, 1, 1, 640000, 1, 40, 40, 1, 16384, 10240, 1280, 838, 10008}},
    {"GENPC_HPR_HOME_CHUNKS=1", {64, 10000, 0, 256, -1, 3072, 1, 1, 1, 0}, {0, 79, 1, 0, 26, 256, 1, 1, 640000, 1, 40, 40, 1, 16384, 10240, 1280, 838, 10008}},
    {"GENPC_HPR_HOME_CHUNKS=4", {64, 10000, 0, 256, -1, 3072, 1, 4, 1, 0}, {0, 79, 1, 0, 26, 256, 1, 4, 640000, 1, 40, 40, 1, 16384, 10240, 1280, 838, 10008}},
    {"GENPC_HPR_HOME_CHUNKS=9 -> 4", {64, 10000, 0, 256, -1, 3072, 1, 9, 1, 0}, {0, 79, 1, 0, 26, 256, 1, 4, 640000, 1, 40, 40, 1, 16384, 10240, 1280, 838, 10008}},
    {"one kernel: both home switches are ignored", {8, 12499, 0, 256, -1, 3072, 1, 1, 1, 0}, {0, 98, 0, 0, 23, 256, 3, 4, 0, 0, 49, 49, 1, 16384, 10240, 1280, 670, 12507}},
    {"GENPC_HPR_DECIDE_KERNEL=0", {64, 10000, 0, 256, -1, 3072, 1, 2, 0, 0}, {0, 79, 1, 0, 26, 256, 1, 2, 640000, 0, 40, 40, 1, 16384, 10240, 1280, 838, 10008}},
    {"GENPC_HPR_NOCULL=128: no decide launch", {64, 10000, 0, 256, -1, 3072, 1, 2, 1, 128}, {0, 79, 1, 0, 26, 256, 1, 2, 640000, 0, 40, 40, 1, 16384, 10240, 1280, 838, 10008}},
    {"GENPC_HPR_NOCULL=512: the decide launch stays", {64, 10000, 0, 256, -1, 3072, 3, 2, 1, 512}, {0, 79, 1, 0, 26, 256, 3, 4, 640000, 1, 40, 40, 1, 16384, 10240, 1280, 838, 10008}},
    {"4096 views are accepted", {4096, 1, 0, 256, -1, 3072, 1, 2, 1, 0}, {0, 1, 0, 0, 32, 256, 3, 4, 0, 0, 1, 1, 16, 4096, 4096, 1280, 1024, 9}},
    {"4097 views", {4097, 1, 0, 256, -1, 3072, 1, 2, 1, 0}, {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}},
    {"2^31 pairs", {2048, 1048576, 0, 256, -1, 3072, 1, 2, 1, 0}, {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}},
    {"2^31 - 2048 pairs are accepted", {2048, 1048575, 0, 256, -1, 3072, 1, 2, 1, 0}, {0, 8192, 0, 0, 31, 48, 3, 4, 0, 0, 4096, 1024, 8, 16384, 10240, 1280, 7, 1048583}},
};

static void table()
{
    for (const Row &r : kTable) row(r.what, r.ask, r.want);
}

static void fail(const HprAsk &a, const char *what, long long v)
{
    if (g_failed++ < 30)
        printf("FAILED %s (%lld): %d x %d, best_only %d, %d CUs, split %d, park %d MiB, home %d / %d\n", what, v, a.c, a.n, a.best_only, a.cus, a.env_split,
               a.env_park_mb, a.env_home_tiles, a.env_home_chunks);
}

// what must hold for every plan, whatever the thresholds are
static void properties()
{
    const int views[] = {1, 2, 3, 7, 8, 9, 64, 1000, 1024, 4096};
    const int sizes[] = {1, 2, 127, 128, 129, 255, 256, 257, 1000, 3001, 10000, 12499, 12500, 16384, 32640, 32641, 100000, 165546, 200000};
    long long seen_split = 0, seen_one = 0, seen_large = 0, seen_pruned = 0;
    for (int c : views)
        for (int n : sizes)
            for (int cus : {64, 256, 304})
                for (int split : {-1, 0, 1})
                    for (int best : {0, 1})
                        for (int mb : {3072, 1, 0})
                            for (int home : {1, 0, 3, 5}) {
                                HprAsk a;
                                a.c = c;
                                a.n = n;
                                a.cus = cus;
                                a.best_only = best;
                                a.env_split = split;
                                a.env_park_mb = mb;
                                a.env_home_tiles = home;
                                a.env_home_chunks = home + 1;
                                const HprPlan p = hpr_plan(a);
                                const long long total = (long long)c * n;
                                if (p.too_large) { fail(a, "too large", total); continue; }
                                if ((long long)p.ntiles * 128 < n || (long long)(p.ntiles - 1) * 128 >= n) fail(a, "tiles do not cover the points", p.ntiles);
                                if ((long long)p.row_grid * 256 < n || (long long)(p.row_grid - 1) * 256 >= n) fail(a, "row grid", p.row_grid);
                                if (p.bounds_grid < 1 || p.bounds_grid > 1024 || p.bounds_grid > p.row_grid) fail(a, "bounds grid", p.bounds_grid);
                                if ((long long)p.view_grid * 256 < c || (long long)(p.view_grid - 1) * 256 >= c) fail(a, "view grid", p.view_grid);
                                if (p.key_bits < 20 || p.key_bits > 32 || (1ll << (p.key_bits - 20)) < c) fail(a, "key bits do not hold the view", p.key_bits);
                                // every wave-per-point grid: at least a block, at most an item's worth (the first try's rounded up to 8)
                                if (p.walk_blocks < 1 || p.walk_blocks > total || p.walk_blocks > 40ll * cus) fail(a, "walk blocks", p.walk_blocks);
                                if (p.large_blocks < 1 || p.large_blocks > total || p.large_blocks > 5ll * cus) fail(a, "large blocks", p.large_blocks);
                                if (p.decide_blocks < 8 || p.decide_blocks % 8 || p.decide_blocks > total + 7 || p.decide_blocks > 64ll * cus + 7) fail(a, "decide blocks", p.decide_blocks);
                                if (p.global_blocks < 1 || p.global_blocks > total || p.global_blocks > 1024) fail(a, "global blocks", p.global_blocks);
                                if (p.gcap != n + 8 || p.global_bytes != (long long)p.global_blocks * 2 * p.gcap * 16) fail(a, "global tier's size", p.global_bytes);
                                if (p.global_bytes > (256ll << 20) && p.global_blocks != 1) fail(a, "global tier over 256 MiB", p.global_bytes);
                                if (p.park_cap > total || (p.split ? p.park_cap < 1 : p.park_cap != 0) || p.park_bytes != p.park_cap * 160) fail(a, "park cap", p.park_cap);
                                if (p.park_bytes > ((long long)(mb > 0 ? mb : 1) << 20) && p.park_cap != 1) fail(a, "polygon store over its MiB", p.park_bytes);
                                if (p.prune && !p.split) fail(a, "views pruned in the one-kernel form", p.prune);
                                if (p.prune != (best && p.split)) fail(a, "prune", p.prune);
                                if (p.home_tiles < 1 || p.home_tiles > 3 || p.home_chunks < 1 || p.home_chunks > 4) fail(a, "home tiles / chunks", p.home_tiles);
                                if (!p.split && (p.home_tiles != 3 || p.home_chunks != 4 || p.decide_kernel)) fail(a, "one-kernel form with the other's settings", p.home_tiles);
                                if (p.home_tiles != 1 && p.home_chunks != 4) fail(a, "chunks of a home tile that is not the only one", p.home_chunks);
                                if (p.max_clips != (p.ntiles >= 256 ? 48 : 256)) fail(a, "max_clips", p.max_clips);
                                if (split < 0 && p.split != (p.ntiles < 256 && total >= 100000 ? 1 : 0)) fail(a, "form by size", p.split);
                                if (p.pairs != total || p.fl_count != 3 * total || p.tile_count != (long long)c * p.ntiles || p.surv_count != (p.split ? total : 0))
                                    fail(a, "element counts", p.pairs);
                                seen_split += p.split != 0;
                                seen_one += !p.split && p.ntiles < 256;
                                seen_large += !p.split && p.ntiles >= 256;
                                seen_pruned += p.prune;
                            }
    if (!seen_split || !seen_one || !seen_large || !seen_pruned) { printf("FAILED: the sweep never met one of the forms\n"); g_failed++; }
}

int main(int argc, char **argv)
{
    g_print = argc > 1 && !strcmp(argv[1], "--exported");
    table();
    if (g_print) return 0;
    // nothing to do is a plan too (the call returns before it launches anything)
    HprAsk z;
    z.c = 5;
    const HprPlan p = hpr_plan(z);
    if (p.too_large || p.ntiles || p.pairs || p.walk_blocks) { printf("FAILED: the plan of an empty cloud\n"); g_failed++; }
    z.c = 1;
    z.n = 0x7fffffff;          // (n + 8 is no int)
    if (!hpr_plan(z).too_large) { printf("FAILED: 2^31 - 1 points\n"); g_failed++; }
    properties();
    if (g_failed) {
        printf("hpr_plan_check: %d check(s) failed\n", g_failed);
        return 1;
    }
    printf("hpr_plan_check: ok\n");
    return 0;
}
