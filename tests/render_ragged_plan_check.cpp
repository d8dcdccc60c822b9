// Stand-alone check of genpc_amd/csrc/render_ragged_plan.h (host code only; tests/test_render_ragged_plan.py builds it with
// -fsanitize=address,undefined and runs it).  Exit status 0 = every check passed; each failure prints what it found.
// What is expected of a width is counted here from the sizes: ceil(n / 256) blocks, at most 1024, at least 1; the backward gather
// serves 32 points a block (eight lanes a point).
// With arguments -- size blend radius n_0 n_1 ... -- it prints the twelve numbers genpc_render_ragged_plan lays out for that list
// (every element with that radius), or "refused" (the Python side compares with the exported function).
#include "render_ragged_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

using namespace genpc;

static int g_failed = 0;

static void expect(const char *what, const char *which, long long got, long long want)
{
    if (got != want) { printf("FAILED %s: %s = %lld, expected %lld\n", what, which, got, want); g_failed++; }
}

static std::vector<int> offsets(const std::vector<int> &n)
{
    std::vector<int> off(n.size() + 1, 0);          // exactly s + 1 entries: the sanitizer sees a read past them
    for (size_t j = 0; j < n.size(); j++) off[j + 1] = off[j] + n[j];
    return off;
}

static int blocks(long long n) { long long g = (n + 255) / 256; return (int)(g > 1024 ? 1024 : (g < 1 ? 1 : g)); }

static RenderRaggedPlan plan_of(const std::vector<int> &n, int size = 64, int blend = 1, bool backward = false, float radius = 0.02f)
{
    const std::vector<int> off = offsets(n);
    const std::vector<float> rad(n.size(), radius);          // exactly s entries
    RenderRaggedAsk a;
    a.s = (int)n.size(); a.off = off.data(); a.radius = rad.data(); a.size = size; a.blend = blend; a.backward = backward;
    return render_ragged_plan(a);
}

static void expect_refused(const char *what, const RenderRaggedPlan &p, const char *why, int element = -1)
{
    if (!p.refuse || strcmp(p.refuse, why) != 0) {
        printf("FAILED %s: refusal = %s, expected %s\n", what, p.refuse ? p.refuse : "(none)", why);
        g_failed++;
    }
    expect(what, "refuse_element", p.refuse_element, element);
    // a refused plan launches nothing and reserves nothing
    expect(what, "gx of a refusal", p.gx, 0);
    expect(what, "g_proj of a refusal", p.g_proj, 0);
    expect(what, "w_pixels of a refusal", (long long)p.w_pixels, 0);
}

static void check_shape(const char *what, const std::vector<int> &n, int size)
{
    int nmax = 0;
    long long total = 0;
    for (int v : n) { nmax = v > nmax ? v : nmax; total += v; }
    const long long s = (long long)n.size();
    for (int backward = 0; backward < 2; backward++) {
        const RenderRaggedPlan p = plan_of(n, size, 1, backward != 0);
        if (p.refuse) { printf("FAILED %s: refused: %s\n", what, p.refuse); g_failed++; continue; }
        expect(what, "s", p.s, s);
        expect(what, "nmax", p.nmax, nmax);
        expect(what, "total", p.total, total);
        expect(what, "pixels", p.pixels, (long long)size * size);
        if (backward && total == 0) {
            expect(what, "nothing", p.nothing, 1);
            expect(what, "gx of nothing", p.gx, 0);
            continue;
        }
        expect(what, "nothing", p.nothing, 0);
        expect(what, "g_proj", p.g_proj, blocks(nmax));
        expect(what, "g_pix", p.g_pix, blocks((long long)size * size));
        expect(what, "gx", p.gx, blocks(8ll * nmax));
        expect(what, "grad_blocks", p.grad_blocks, (long long)blocks(8ll * nmax) * s);
        // every point of the largest element has its eight lanes within one pass of gx blocks, or the blocks loop (the cap)
        if (p.gx < 1024) expect(what, "gx covers nmax", (long long)p.gx * 32 >= nmax, 1);
        expect(what, "nmax_piece holds the total", (long long)p.nmax_piece * s >= total && p.nmax_piece >= 1, 1);
        expect(what, "nmax_piece is the least such", p.nmax_piece == 1 || ((long long)p.nmax_piece - 1) * s < total, 1);
        expect(what, "table_ints", (long long)p.table_ints, s + 1);
        expect(what, "table_floats", (long long)p.table_floats, s);
        expect(what, "w_pixels", (long long)p.w_pixels, s * size * size);
    }
}

static int print_plan(int argc, char **argv)
{
    const int size = atoi(argv[1]), blend = atoi(argv[2]);
    const float radius = (float)atof(argv[3]);
    std::vector<int> n;
    for (int k = 4; k < argc; k++) n.push_back(atoi(argv[k]));
    const RenderRaggedPlan p = plan_of(n, size, blend, false, radius);
    if (p.refuse) {
        char why[128];
        render_ragged_refusal(p, why, sizeof why);
        printf("refused %d %s\n", p.refuse_element, why);
        return 0;
    }
    const long long cap = 0x7fffffffll;
    const long long out[12] = {kRenderRaggedMax, -1, p.s, p.nmax, std::min(p.total, cap), p.pixels, p.g_proj, p.g_pix, p.gx,
                               std::min(p.grad_blocks, cap), std::min((long long)p.nmax_piece, cap), std::min((long long)p.w_pixels, cap)};
    for (int k = 0; k < 12; k++) printf("%lld ", out[k]);
    printf("\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 4) return print_plan(argc, argv);

    // ---- refusals, in the order they are asked
    {
        RenderRaggedAsk a;
        const int off2[3] = {0, 5, 9};
        const float rad2[2] = {0.01f, 0.02f};
        a.off = off2; a.radius = rad2; a.size = 64; a.blend = 1;
        a.s = 0;
        expect_refused("s = 0", render_ragged_plan(a), "s must be positive");
        a.s = -3;
        expect_refused("s < 0", render_ragged_plan(a), "s must be positive");
        a.s = kRenderRaggedMax + 1;          // (refused before either table is read: they hold two elements)
        expect_refused("s over the bound", render_ragged_plan(a), "more than 384 elements in one call");
        a.s = 2;
        a.off = nullptr;
        expect_refused("off null", render_ragged_plan(a), "off is null");
        a.off = off2; a.radius = nullptr;
        expect_refused("radius null", render_ragged_plan(a), "radius is null");
        a.radius = rad2;
        for (int size : {0, -1, 8193}) {
            a.size = size;
            expect_refused("size", render_ragged_plan(a), "size must be in 1 .. 8192");
        }
        a.size = 64;
        for (int blend : {-1, 2}) {
            a.blend = blend;
            expect_refused("blend", render_ragged_plan(a), "blend must be 0 or 1");
        }
        a.blend = 0;
        const int start1[3] = {1, 5, 9}, desc[3] = {0, 5, 4};
        a.off = start1;
        expect_refused("table starts at 1", render_ragged_plan(a), "offsets must start at 0");
        a.off = desc;
        expect_refused("table descends", render_ragged_plan(a), "offsets must ascend");
        a.off = off2;
        const float zero1[2] = {0.01f, 0.0f}, neg0[2] = {-1.0f, 0.02f}, nan1[2] = {0.01f, __builtin_nanf("")};
        a.radius = zero1;
        expect_refused("radius 0", render_ragged_plan(a), "the radius of every element must be positive", 1);
        a.radius = neg0;
        expect_refused("radius < 0", render_ragged_plan(a), "the radius of every element must be positive", 0);
        a.radius = nan1;
        expect_refused("radius NaN", render_ragged_plan(a), "the radius of every element must be positive", 1);
        {
            char why[128];
            render_ragged_refusal(render_ragged_plan(a), why, sizeof why);
            if (strcmp(why, "the radius of every element must be positive (element 1)") != 0) { printf("FAILED refusal text: %s\n", why); g_failed++; }
        }
        a.radius = rad2;
        const int big[3] = {0, 5, (1 << 28) + 1}, most[3] = {0, 5, 1 << 28};
        a.off = big;
        expect_refused("off[s] over 2^28", render_ragged_plan(a), "off[s] and s * size * size must not exceed 2^28");
        a.off = most;
        expect("off[s] = 2^28", "taken", render_ragged_plan(a).refuse == nullptr, 1);
        a.off = off2;
        a.size = 8192;          // 2 x 2^26 pixels: taken; 5 elements: refused
        expect("s * size * size = 2^27", "taken", render_ragged_plan(a).refuse == nullptr, 1);
        {
            const int off5[6] = {0, 1, 2, 3, 4, 5};
            const float rad5[5] = {1, 1, 1, 1, 1};
            RenderRaggedAsk b = a;
            b.s = 5; b.off = off5; b.radius = rad5;
            expect_refused("s * size * size over 2^28", render_ragged_plan(b), "off[s] and s * size * size must not exceed 2^28");
            b.s = 4;
            expect("s * size * size = 2^28", "taken", render_ragged_plan(b).refuse == nullptr, 1);
        }
        a.size = 64;
        // null device pointers with work to do
        a.img = false;
        expect_refused("img null", render_ragged_plan(a), "img is null");
        a.img = true; a.pts = false;
        expect_refused("pts null, forward", render_ragged_plan(a), "pts is null");
        const int none[3] = {0, 0, 0};
        a.off = none;
        expect("pts null without points", "taken", render_ragged_plan(a).refuse == nullptr, 1);
        a.backward = true;
        expect("backward without points", "nothing", render_ragged_plan(a).nothing, 1);
        expect("backward without points", "taken", render_ragged_plan(a).refuse == nullptr, 1);
        a.off = off2;
        expect_refused("pts null, backward", render_ragged_plan(a), "pts is null");
        a.pts = true; a.planes = false;
        expect_refused("planes null", render_ragged_plan(a), "planes is null");
        a.planes = true; a.grad_img = false;
        expect_refused("grad_img null", render_ragged_plan(a), "grad_img is null");
        a.grad_img = true; a.grad_pts = false;
        expect_refused("grad_pts null", render_ragged_plan(a), "grad_pts is null");
        a.grad_pts = true; a.img = false;          // (the backward has no img)
        expect("backward, complete", "taken", render_ragged_plan(a).refuse == nullptr, 1);
    }

    // ---- s at the bound and one over
    {
        std::vector<int> n(kRenderRaggedMax, 3);
        check_shape("s at the bound", n, 32);
        n.push_back(3);
        expect_refused("s one over the bound", plan_of(n, 32), "more than 384 elements in one call");
    }

    // ---- empty elements only; the largest element first, last and in the middle
    check_shape("one empty element", {0}, 64);
    check_shape("empty elements only", {0, 0, 0}, 64);
    check_shape("largest first", {2451, 31, 0, 257}, 96);
    check_shape("largest last", {31, 0, 257, 2451}, 96);
    check_shape("largest in the middle", {31, 2451, 0, 257}, 96);
    expect("largest first / last", "same grids", plan_of({2451, 31, 0, 257}, 96).gx == plan_of({31, 0, 257, 2451}, 96).gx, 1);

    // ---- the grids for largest elements of 1, 32, 33, 256, 257 points (the gather: 32 points a block; the projection: 256)
    {
        const int nmax[5] = {1, 32, 33, 256, 257}, gx[5] = {1, 1, 2, 8, 9}, gp[5] = {1, 1, 1, 1, 2};
        for (int k = 0; k < 5; k++) {
            char what[64];
            snprintf(what, sizeof what, "largest element of %d", nmax[k]);
            const RenderRaggedPlan p = plan_of({0, nmax[k], 1}, 64, 0, true);
            expect(what, "gx", p.gx, gx[k]);
            expect(what, "g_proj", plan_of({0, nmax[k], 1}, 64, 0, false).g_proj, gp[k]);
            expect(what, "grad_blocks", p.grad_blocks, 3ll * gx[k]);
            check_shape(what, {0, nmax[k], 1}, 64);
        }
        // the cap: 1024 blocks per element whatever the size
        expect("a large element", "gx", plan_of({1 << 20}, 64, 0, true).gx, 1024);
        expect("a large element", "g_proj", plan_of({1 << 20}, 64).g_proj, 1024);
        expect("a large image", "g_pix", plan_of({5}, 8192).g_pix, 1024);
        expect("one pixel", "g_pix", plan_of({5}, 1).g_pix, 1);
    }

    if (g_failed) { printf("render_ragged_plan_check: %d FAILED\n", g_failed); return 1; }
    printf("render_ragged_plan_check: ok\n");
    return 0;
}
