// Stand-alone check of genpc_amd/csrc/pose_ragged_plan.h (host code only; tests/test_pose_ragged_plan.py builds it with
// -fsanitize=address,undefined and runs it).  Exit status 0 = every check passed; each failure prints what it found.
// What is expected of a width is counted here from the sizes (ceil(n / 256), at most 1024), of a choice taken over from
// pose_plan.h by asking pose_plan.h itself -- no second copy of its thresholds.
#include "pose_ragged_plan.h"

#include <stdio.h>
#include <string.h>
#include <vector>

using namespace genpc;

static int g_failed = 0;

static void expect(const char *what, const char *which, long long got, long long want)
{
    if (got != want) { printf("FAILED %s: %s = %lld, expected %lld\n", what, which, got, want); g_failed++; }
}

static std::vector<int> offsets(const std::vector<int> &n)
{
    std::vector<int> off(n.size() + 1, 0);          // exactly c + 1 entries: the sanitizer sees a read past them
    for (size_t j = 0; j < n.size(); j++) off[j + 1] = off[j] + n[j];
    return off;
}

static PoseRaggedPlan plan_of(const std::vector<int> &nc, const std::vector<int> &np, int starts, bool mask, int size = 224, float radius = 0.02f)
{
    const std::vector<int> coff = offsets(nc), poff = offsets(np);
    PoseRaggedAsk a;
    a.c = (int)nc.size(); a.coff = coff.data(); a.poff = poff.data(); a.starts = starts; a.mask = mask; a.render_size = size; a.radius = radius;
    a.cus = 256;
    return pose_ragged_plan(a);
}

static int blocks(long long n) { long long g = (n + 255) / 256; return (int)(g > 1024 ? 1024 : (g < 1 ? 1 : g)); }

int main()
{
    // element numbering: e = scan * starts + start; the element tables ascend and partition the starts-fold packed arrays
    for (int starts : {1, 4}) {
        const std::vector<int> n = {5, 700, 63};
        const std::vector<int> off = offsets(n);
        std::vector<int> e(n.size() * starts + 1, -1);
        pose_ragged_element_offsets((int)n.size(), off.data(), starts, e.data());
        char what[64];
        snprintf(what, sizeof what, "element table, %d start(s)", starts);
        expect(what, "first", e[0], 0);
        expect(what, "last", e[n.size() * starts], (long long)starts * off[n.size()]);
        for (size_t j = 0; j < n.size(); j++)
            for (int s = 0; s < starts; s++) {
                const size_t el = j * starts + s;
                expect(what, "count of an element", e[el + 1] - e[el], n[j]);
                expect(what, "base of an element", e[el], (long long)starts * off[j] + (long long)s * n[j]);
            }
        const PoseRaggedPlan p = plan_of(n, {3, 300, 257}, starts, false);
        expect(what, "elements", p.elements, 3 * starts);
        expect(what, "replicate", p.replicate, starts > 1);
        expect(what, "total_c", p.total_c, (long long)starts * 768);
        expect(what, "total_p", p.total_p, (long long)starts * 560);
    }
    // n_max: wherever the largest cloud stands, each side by itself
    {
        const PoseRaggedPlan p = plan_of({5, 63, 64, 257, 700, 300}, {3, 257, 64, 63, 300, 700}, 1, true, 48, 0.05f);
        expect("six pairs", "nc_max", p.nc_max, 700);
        expect("six pairs", "np_max", p.np_max, 700);
        expect("six pairs", "g_t", p.g_t, blocks(700));
        expect("six pairs", "g_g", p.g_g, blocks(1400));
        expect("six pairs", "g_m", p.g_m, blocks(700));
        expect("six pairs", "gb", p.gb, 1);
        expect("six pairs", "ride", p.ride, 1);                      // one stream, full objective
        expect("six pairs", "nmax_piece covers the totals", (long long)p.nmax_piece * p.elements >= 1389, 1);
        const PoseRaggedPlan r = plan_of({300, 700, 257, 64, 63, 5}, {700, 300, 63, 64, 257, 3}, 1, true, 48, 0.05f);
        expect("six pairs reversed", "nc_max", r.nc_max, 700);
        expect("six pairs reversed", "g_g", r.g_g, p.g_g);
        expect("six pairs reversed", "sub8", r.step.sub8, p.step.sub8);
        expect("six pairs reversed", "fuse_w", r.step.fuse_w, p.step.fuse_w);
    }
    // a one-point scan: every width is one block, and the step's choices are mask_step_plan's for that one point
    {
        const PoseRaggedPlan p = plan_of({1}, {1}, 1, true);
        const MaskStepPlan m = mask_step_plan(1, 1, 224, 0.02f);
        expect("one point", "elements", p.elements, 1);
        expect("one point", "g_t", p.g_t, 1);
        expect("one point", "g_g", p.g_g, 1);
        expect("one point", "g_m", p.g_m, 1);
        expect("one point", "g_rep", p.g_rep, 1);
        expect("one point", "gb", p.gb, 1);
        expect("one point", "gp", p.step.gp, m.gp);
        expect("one point", "gs", p.step.gs, m.gs);
        expect("one point", "fuse_w", p.step.fuse_w, m.fuse_w);
        expect("one point", "sub8", p.step.sub8, m.sub8);
        expect("one point", "too_large", p.too_large != nullptr, 0);
    }
    // a call of one size is the equal-size loop's plan for that size on one stream
    {
        const std::vector<int> nc(16, 4493), np(16, 886);
        const PoseRaggedPlan p = plan_of(nc, np, 4, true);
        PoseLoopAsk la;
        la.scans = 64; la.starts = 1; la.nc = 4493; la.np = 886; la.mask = true; la.side_stream_ok = false; la.counters_ok = false;
        const PoseLoopPlan lp = pose_loop_plan(la);
        const MaskStepPlan m = mask_step_plan(64, 4493, 224, 0.02f);
        expect("16 scans x 4 starts", "elements", p.elements, 64);
        expect("16 scans x 4 starts", "g_t", p.g_t, lp.g_t);
        expect("16 scans x 4 starts", "g_g", p.g_g, lp.g_g);
        expect("16 scans x 4 starts", "g_g is capped", p.g_g, 22);      // ceil(5379 / 256) = 22 < 24
        expect("16 scans x 4 starts", "gb", p.gb, lp.gb);
        expect("16 scans x 4 starts", "ride", p.ride, lp.ride);
        expect("16 scans x 4 starts", "fuse_w", p.step.fuse_w, m.fuse_w);
        expect("16 scans x 4 starts", "sub8", p.step.sub8, m.sub8);
        expect("16 scans x 4 starts", "blocks_per_cu", p.blocks_per_cu, (18 * 64 + 255) / 256);
        expect("16 scans x 4 starts", "wants no side stream either", pose_wants_side(la) && 64ll * 4493 <= 65536, 0);
    }
    // the step's choices come from the totals (the mean element), not from the largest element
    {
        std::vector<int> nc(12, 100), np(12, 100);
        nc[5] = 30000;          // mean (1100 + 30000) / 12 = 2592: 12 x 2592 = 31104 > 24576 -> one lane per point
        const PoseRaggedPlan p = plan_of(nc, np, 1, true);
        const MaskStepPlan mean = mask_step_plan(12, 2592, 224, 0.02f), largest = mask_step_plan(12, 30000, 224, 0.02f);
        expect("one large element", "nc_max", p.nc_max, 30000);
        expect("one large element", "sub8 of the mean", p.step.sub8, mean.sub8);
        expect("one large element", "fuse_w of the mean", p.step.fuse_w, mean.fuse_w);
        expect("one large element", "the mean and the largest disagree on fuse_w", mean.fuse_w != largest.fuse_w, 1);
        expect("one large element", "g_t is for the largest", p.g_t, blocks(30000));
    }
    // 384 elements: the most a call holds, as scans x starts
    {
        const std::vector<int> nc(96, 4493), np(96, 886);
        const PoseRaggedPlan p = plan_of(nc, np, 4, true);
        expect("96 scans x 4 starts", "too_large", p.too_large != nullptr, 0);
        expect("96 scans x 4 starts", "elements", p.elements, 384);
        expect("96 scans x 4 starts", "gb", p.gb, 6);
        expect("96 scans x 4 starts", "g_t", p.g_t, blocks(4493));
        expect("96 scans x 4 starts", "g_g", p.g_g, 22);
        expect("96 scans x 4 starts", "total_c", p.total_c, 4ll * 96 * 4493);
        const std::vector<int> one(384, 1);
        const PoseRaggedPlan q = plan_of(one, one, 1, false);
        expect("384 scans x 1 start", "too_large", q.too_large != nullptr, 0);
        expect("384 scans x 1 start", "elements", q.elements, 384);
        expect("384 scans x 1 start", "ride", q.ride, 0);               // Chamfer only: nothing to ride in
        std::vector<int> e(385, -1);
        const std::vector<int> off = offsets(one);
        pose_ragged_element_offsets(384, off.data(), 1, e.data());
        expect("384 scans x 1 start", "last table entry", e[384], 384);
    }
    // 385: refused, with a message that says so, before a size is looked at
    {
        const std::vector<int> one(385, 1);
        const PoseRaggedPlan p = plan_of(one, one, 1, false);
        expect("385 scans", "too_large", p.too_large != nullptr, 1);
        if (p.too_large && !strstr(p.too_large, "384 elements")) { printf("FAILED 385 scans: message '%s'\n", p.too_large); g_failed++; }
        const std::vector<int> n97(97, 10);
        const PoseRaggedPlan q = plan_of(n97, n97, 4, true);
        expect("97 scans x 4 starts", "too_large", q.too_large != nullptr, 1);
        const int off2[2] = {0, 1};
        PoseRaggedAsk a;
        a.c = 1; a.coff = off2; a.poff = off2; a.starts = 385;
        expect("1 scan x 385 starts", "too_large", pose_ragged_plan(a).too_large != nullptr, 1);
    }
    // totals that overflow kRaggedMaxPoints: the starts count (the offsets themselves stay ints)
    {
        const int big[3] = {0, kRaggedMaxPoints / 4, kRaggedMaxPoints / 2};
        const int small[3] = {0, 1, 2};
        PoseRaggedAsk a;
        a.c = 2; a.coff = big; a.poff = small; a.starts = 2;
        const PoseRaggedPlan ok = pose_ragged_plan(a);
        expect("2^27 x 2 starts", "too_large", ok.too_large != nullptr, 0);
        expect("2^27 x 2 starts", "total_c", ok.total_c, kRaggedMaxPoints);
        a.starts = 4;
        const PoseRaggedPlan p = pose_ragged_plan(a);
        expect("2^27 x 4 starts", "too_large", p.too_large != nullptr, 1);
        if (p.too_large && !strstr(p.too_large, "2^28 points")) { printf("FAILED 2^27 x 4 starts: message '%s'\n", p.too_large); g_failed++; }
        a.coff = small; a.poff = big; a.starts = 3;
        expect("partial side, 3 starts", "too_large", pose_ragged_plan(a).too_large != nullptr, 1);
        const int most[2] = {0, 0x7fffffff};
        a.c = 1; a.coff = most; a.poff = small; a.starts = 384;          // (the product needs 64 bits)
        expect("2^31 x 384 starts", "too_large", pose_ragged_plan(a).too_large != nullptr, 1);
    }
    // c = 0: nothing, and the tables are not looked at
    {
        PoseRaggedAsk a;
        a.c = 0; a.starts = 4; a.mask = true; a.render_size = 224; a.radius = 0.02f;
        const PoseRaggedPlan p = pose_ragged_plan(a);
        expect("no scan", "elements", p.elements, 0);
        expect("no scan", "too_large", p.too_large != nullptr, 0);
        expect("no scan", "widths", p.g_t + p.g_g + p.gb + p.g_m, 0);
    }
    // two element tables of 385 ints and what else the tables kernel takes fit the 4 KiB of kernel arguments
    if (sizeof(RaggedTable) + 8 * sizeof(void *) + 16 > 4096) { printf("FAILED: the tables do not fit the kernel arguments\n"); g_failed++; }

    if (g_failed) {
        printf("pose_ragged_plan_check: %d check(s) failed\n", g_failed);
        return 1;
    }
    printf("pose_ragged_plan_check: ok\n");
    return 0;
}
