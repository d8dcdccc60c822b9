// Stand-alone check of genpc_amd/csrc/pose_plan.h (host code only; tests/test_pose_plan.py builds it with
// -fsanitize=address,undefined and runs it).  Exit status 0 = every row passed; each failure prints its row and field.
// A table of asks with the plan each must give, written as literals worked out by hand from the conditions as they stood in
// genpc_pose_optimize_batch and mask_step before the header existed -- no second copy of the expressions.  A field a row does
// not pin is kAny.  Rows at the exact fuse_w boundary are deliberately absent: that expression is fp32 / fp64 mixed.
#include "pose_plan.h"

#include <stdio.h>

using namespace genpc;

static int g_failed = 0;
constexpr int kAny = -99;

struct Want {
    int lock = kAny, elements = kAny, starts_left = kAny, dual = kAny, flags = kAny, fuse_upd = kAny, ride = kAny, seed_mode = kAny,
        g_t = kAny, g_g = kAny, gb = kAny;
};

static void field(const char *row, const char *name, int got, int want)
{
    if (want != kAny && got != want) { printf("FAILED %s: %s = %d, expected %d\n", row, name, got, want); g_failed++; }
}

static void row(const char *name, const PoseLoopAsk &a, const Want &w)
{
    const PoseLoopPlan p = pose_loop_plan(a);
    field(name, "lock", p.lock, w.lock);
    field(name, "elements", p.elements, w.elements);
    field(name, "starts_left", p.starts_left, w.starts_left);
    field(name, "dual", p.dual, w.dual);
    field(name, "flags", p.flags, w.flags);
    field(name, "fuse_upd", p.fuse_upd, w.fuse_upd);
    field(name, "ride", p.ride, w.ride);
    field(name, "seed_mode", p.seed_mode, w.seed_mode);
    field(name, "g_t", p.g_t, w.g_t);
    field(name, "g_g", p.g_g, w.g_g);
    field(name, "gb", p.gb, w.gb);
    // the wish for a side stream is what the loop asks before it has one: the same whatever came back
    PoseLoopAsk none = a;
    none.side_stream_ok = none.counters_ok = false;
    if (pose_wants_side(a) != pose_wants_side(none) || p.wants_side != pose_wants_side(a)) { printf("FAILED %s: wants_side depends on what was delivered\n", name); g_failed++; }
    if (p.dual && !p.wants_side) { printf("FAILED %s: dual without the wish\n", name); g_failed++; }
}

static PoseLoopAsk ask(int scans, int starts, int nc, int np, bool mask)
{
    PoseLoopAsk a;          // switches at their defaults, modes unset, side stream and counters there, no serialising tool
    a.scans = scans; a.starts = starts; a.nc = nc; a.np = np; a.mask = mask;
    return a;
}

static Want want(int lock, int elements, int starts_left, int dual, int flags, int fuse_upd, int ride, int seed_mode, int g_t, int g_g, int gb)
{
    Want w;
    w.lock = lock; w.elements = elements; w.starts_left = starts_left; w.dual = dual; w.flags = flags; w.fuse_upd = fuse_upd; w.ride = ride;
    w.seed_mode = seed_mode; w.g_t = g_t; w.g_g = g_g; w.gb = gb;
    return w;
}

static void mask_row(const char *name, int elements, int nc, int S, float radius, int gp, int gs, int fuse_w, int sub8)
{
    const MaskStepPlan p = mask_step_plan(elements, nc, S, radius);
    field(name, "gp", p.gp, gp);
    field(name, "gs", p.gs, gs);
    field(name, "fuse_w", p.fuse_w, fuse_w);
    field(name, "sub8", p.sub8, sub8);
}

int main()
{
    // lin_grid: blocks of 256, 1 .. 1024
    field("lin_grid", "0", lin_grid(0), 1);
    field("lin_grid", "256", lin_grid(256), 1);
    field("lin_grid", "257", lin_grid(257), 2);
    field("lin_grid", "262144", lin_grid(262144), 1024);
    field("lin_grid", "2^33", lin_grid(1ll << 33), 1024);

    // the test clouds of tests/test_gpu_pose_update_forms.py: 4 elements x 1200 = 4800 points <= 65536: a side stream, and with
    // it the filter (the wish switches the adaptive search off); 4 <= 8 elements: fused update, so counters; dual: nothing rides.
    // g_t = ceil(1200 / 256) = 5, g_g = ceil(1800 / 256) = 8
    const PoseLoopAsk first = ask(1, 4, 1200, 600, true);
    const Want first_want = want(4, 4, 1, 1, 1, 1, 0, 0, 5, 8, 1);
    row("1x4 1200x600 mask", first, first_want);
    // without the mask: no side stream, no fused update (both are the full objective's), nothing to ride in; mode 2 falls to the
    // 24576 gate (4800 points)
    row("1x4 1200x600 cd only", ask(1, 4, 1200, 600, false), want(4, 4, 1, 0, 0, 0, 0, 0, 5, 8, 1));
    // elements x nc = 65536, the side stream's boundary (<=): g_t = 64, g_g = ceil(24576 / 256) = 96
    row("1x4 16384x8192 mask", ask(1, 4, 16384, 8192, true), want(4, 4, 1, 1, 1, 1, 0, 0, 64, 96, 1));
    // one point more per element: 65540 > 65536 no side stream, so pose_grad rides; no wish and 65540 > 24576: mode 2 stays
    row("1x4 16385x8192 mask", ask(1, 4, 16385, 8192, true), want(4, 4, 1, 0, 0, 1, 1, 2, 65, 97, 1));
    // 32 elements: > 8 no fused update, >= 16 at most 24 blocks per element in pose_grad
    row("8x4 16384x8192 mask", ask(8, 4, 16384, 8192, true), want(4, 32, 1, 0, 0, 0, 1, 2, 64, 24, 1));
    // 256 elements, lock-step's boundary (<=)
    {
        Want w;
        w.lock = 4; w.elements = 256; w.starts_left = 1; w.gb = 4;
        row("64x4 300x300 mask", ask(64, 4, 300, 300, true), w);
    }
    // 260 > 256: the starts one after the other, 65 elements: 65 x 300 = 19500 points: a side stream, but no fused update
    // (65 > 8), so its hand-over is by events; g_g = min(24, ceil(600 / 256) = 3)
    row("65x4 300x300 mask", ask(65, 4, 300, 300, true), want(0, 65, 4, 1, 0, 0, 0, 0, 2, 3, 2));
    {   // the grids of the seeded search hold clouds of 256 points and more, whatever the thread asks for
        PoseLoopAsk a = ask(1, 4, 255, 600, false);
        a.t_pose_seeded = 1;
        Want w;
        w.seed_mode = 0;
        row("1x4 255x600 seeded 1", a, w);
        a = ask(1, 4, 600, 255, true);
        a.t_pose_seeded = 2;
        row("1x4 600x255 seeded 2", a, w);
    }
    {   // a thread that asks for a mode gets it at any size: neither size gate applies
        PoseLoopAsk a = first;
        a.t_pose_seeded = 2;
        Want w = first_want;
        w.seed_mode = 2;
        row("first, seeded 2", a, w);
        a.t_pose_seeded = 1;
        w.seed_mode = 1;
        row("first, seeded 1", a, w);
        a.t_pose_seeded = 0;
        w.seed_mode = 0;
        row("first, seeded 0", a, w);
    }
    {   // the thread switches the side stream off: one stream, pose_grad rides; mode 2 falls to the 24576 gate (4800 points)
        PoseLoopAsk a = first;
        a.t_pose_dual = 0;
        row("first, dual 0", a, want(4, 4, 1, 0, 0, 1, 1, 0, 5, 8, 1));
        // ... and the thread's word goes before the switch's
        a.t_pose_dual = 1;
        a.env_dual = 0;
        row("first, dual 1 over GENPC_POSE_DUAL=0", a, first_want);
    }
    {   // the wish without its fulfilment: one stream -- and still the filter (it is the WISH that switches the adaptive search off;
        // here the 24576 gate would do it too, so a second row above that gate: 4 x 8000 = 32000 points)
        PoseLoopAsk a = first;
        a.side_stream_ok = false;
        a.counters_ok = false;
        row("first, no side stream", a, want(4, 4, 1, 0, 0, 1, 1, 0, 5, 8, 1));
        a = ask(1, 4, 8000, 4000, true);
        a.side_stream_ok = false;
        Want w;
        w.dual = 0; w.ride = 1; w.seed_mode = 0;
        row("1x4 8000x4000 mask, no side stream", a, w);
        a.mask = false;          // (no wish: nothing stands between mode 2 and these 32000 points)
        w.ride = 0; w.seed_mode = 2;
        row("1x4 8000x4000 cd only", a, w);
    }
    {   // a side stream without its counters, or under a tool that runs one kernel at a time: events
        PoseLoopAsk a = first;
        Want w = first_want;
        w.flags = 0;
        a.counters_ok = false;
        row("first, no counters", a, w);
        a = first;
        a.serialised_tool = true;
        row("first, serialised tool", a, w);
    }
    // The six switches at 0, each on an ask where it decides something.
    {   // GENPC_POSE_LOCKSTEP: the starts one after the other, one element; the rest as it was
        PoseLoopAsk a = first;
        a.env_lock = 0;
        row("GENPC_POSE_LOCKSTEP=0", a, want(0, 1, 4, 1, 1, 1, 0, 0, 5, 8, 1));
    }
    {   // GENPC_POSE_SEEDED: on the first ask the wish for a side stream has switched mode 2 off already, so 0 changes nothing
        // there and 1 is what shows; 0 shows on the ask whose default is 2
        PoseLoopAsk a = first;
        a.env_seeded = 0;
        row("GENPC_POSE_SEEDED=0", a, first_want);
        a.env_seeded = 1;
        Want w = first_want;
        w.seed_mode = 1;
        row("GENPC_POSE_SEEDED=1", a, w);
        a = ask(1, 4, 16385, 8192, true);
        a.env_seeded = 0;
        row("GENPC_POSE_SEEDED=0, 1x4 16385x8192", a, want(4, 4, 1, 0, 0, 1, 1, 0, 65, 97, 1));
    }
    {   // GENPC_POSE_DUAL: one stream (and what follows from it: no counters, pose_grad rides)
        PoseLoopAsk a = first;
        a.env_dual = 0;
        row("GENPC_POSE_DUAL=0", a, want(4, 4, 1, 0, 0, 1, 1, 0, 5, 8, 1));
    }
    {   // GENPC_POSE_FUSE_UPDATE: the update a launch of its own (and no counters: it is the fused update that waits for them)
        PoseLoopAsk a = first;
        a.env_fuse_upd = 0;
        row("GENPC_POSE_FUSE_UPDATE=0", a, want(4, 4, 1, 1, 0, 0, 0, 0, 5, 8, 1));
    }
    {   // GENPC_POSE_DUAL_FLAGS: events
        PoseLoopAsk a = first;
        a.env_dual_flags = 0;
        row("GENPC_POSE_DUAL_FLAGS=0", a, want(4, 4, 1, 1, 0, 1, 0, 0, 5, 8, 1));
    }
    {   // GENPC_POSE_GRAD_RIDES: with a side stream nothing rides anyway; it shows on one stream
        PoseLoopAsk a = first;
        a.env_ride = 0;
        row("GENPC_POSE_GRAD_RIDES=0", a, first_want);
        a.t_pose_dual = 0;
        row("GENPC_POSE_GRAD_RIDES=0, dual 0", a, want(4, 4, 1, 0, 0, 1, 0, 0, 5, 8, 1));
    }
    {   // one start: nothing to run side by side, whatever the switch says
        PoseLoopAsk a = ask(3, 1, 1200, 600, true);
        Want w;
        w.lock = 0; w.elements = 3; w.starts_left = 1;
        row("3x1", a, w);
        a.env_lock = 0;
        row("3x1 GENPC_POSE_LOCKSTEP=0", a, w);
    }

    // mask_step_plan.  S 224: gp = ceil(50176 / 256) = 196, gs = min(196, 48).  A disc of radius 1.1 x 0.02 is
    // rho = 112 x 4 x 0.022 / 3 = 3.29 pixels, pi rho^2 = 33.9: 2451 points touch 83 k pixels <= 3.5 x 50176 = 176 k, 16384 points 555 k
    mask_row("S 224 r 0.02 4 x 2451", 4, 2451, 224, 0.02f, 196, 48, 1, 1);
    mask_row("S 224 r 0.02 4 x 16384", 4, 16384, 224, 0.02f, 196, 48, 0, 0);
    // eight lanes per point up to 24576 points per launch (<=), or with one or two elements whatever their size
    mask_row("4 x 6144", 4, 6144, 224, 0.02f, kAny, kAny, kAny, 1);
    mask_row("4 x 6145", 4, 6145, 224, 0.02f, kAny, kAny, kAny, 0);
    mask_row("2 x 100000", 2, 100000, 224, 0.02f, kAny, kAny, kAny, 1);
    mask_row("3 x 100000", 3, 100000, 224, 0.02f, kAny, kAny, kAny, 0);
    // S 64: gp = 4096 / 256 = 16 < 48
    mask_row("S 64", 4, 2451, 64, 0.02f, 16, 16, kAny, kAny);

    if (g_failed) {
        printf("pose_plan_check: %d check(s) failed\n", g_failed);
        return 1;
    }
    printf("pose_plan_check: ok\n");
    return 0;
}
