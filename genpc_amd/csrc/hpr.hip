// hpr.hip -- exact hidden-point removal: the operator the reference applies per
// viewpoint through open3d's PointCloud.hidden_point_removal(camera, radius) (DepthPrompting.py:273-290;
// Katz, Tal, Basri 2007): spherical flipping p' = v + 2 (radius - |v|) v / |v| with v = p - camera, then
// the convex hull of the flipped points and the origin; visible = the hull's vertices.
//
// No hull is built here.  A flipped point p'_i is a hull vertex iff some plane through it has every other
// flipped point and the origin strictly on one side, i.e. iff there is a normal n with n.p'_i > 0 and
// n.p'_j < n.p'_i for all j.  n.p'_i > 0 lets n be scaled to n = u + a e1 + b e2 (u = p'_i / |p'_i|;
// e1, e2 an orthonormal basis of u's normal plane); then n.p'_i = |p'_i| and every other point is ONE
// LINEAR constraint on (a, b):
//       a (e1.p'_j) + b (e2.p'_j) <= |p'_i| - u.p'_j
// The feasible (a, b) are a convex polygon -- the cross-section of the vertex's normal cone; for the
// reference's large radii it is the power cell of point i among the cloud's directions, weighted by depth --
// and the point is visible iff the polygon survives clipping by every other point.
//
// Pipeline (one call = all viewpoints; this file: the call, hpr_plan.h: its plan, hpr.h: what the passes share):
//   hpr_order.hip
//   hpr_bounds / hpr_key / rocprim sort  per view, the points in 2-D Morton order of their DIRECTION from the
//                         eye: a surface and what it hides become neighbours, so a hidden point meets its
//                         occluders at once.  The order never changes a result, only when it is reached.
//   hpr_flip_kernel       p' per (view, position), fp64
//   hpr_tile_kernel       per tile of 128 consecutive positions: axis, half-angle, largest |p'| of its directions
//   hpr_accept.hip
//   hpr_accept_kernel     u itself separates (u.p'_j < |p'_i| for all j: the origin of the (a, b) plane strictly
//                         feasible): visible, no polygon -- one dot product per candidate
//   hpr_compact_kernel    the left-over positions per view, in order
//   hpr_first.hip
//   hpr_kernel            one thread per left-over (view, point), polygon in LDS ([vertex][thread], <= kHprMaxV):
//                         (1) the point's home tile, the next, the previous; (2) one interior point of the
//                         polygon tried as THE normal against everything (strictly feasible: visible);
//                         (3) a few batches of the other tiles outward from the group's tile (tiles whose cone
//                         cannot reach the polygon skipped whole, candidates filtered by two reach bounds, then
//                         clipped); whatever is undecided then -- and, for clouds under 256 tiles, everything
//                         undecided after (2), with its polygon saved -- goes to
//   hpr_wave.hip
//   hpr_overflow_kernel   one WAVE per point (also: polygons that outgrow kHprMaxV): 64 candidates tested against
//                         the polygon at a time, clips by all lanes; 128-vertex polygons first, larger ones in a
//                         second launch
// Every skip and every early decision is conservative (margins 1e-7 .. 1e-10 against fp64 roundoff of 1e-16),
// so the mask is that of clipping every polygon by every point.
//
// All arithmetic is double with contraction OFF and the operation order of oracle/genpc_oracle_hpr.c, which
// restates the ordering, the accept test, the grouping and the candidate order: the two produce the same
// polygons bit for bit, hence the same mask.  That restatement is pinned against qhull (scipy) on random clouds,
// real scans and lattices.  Deviations from the hull definition: normals tilted from u by more than atan(1e4)
// are not considered; of exact duplicates only the lowest-index copy takes part (qhull keeps one copy too).
//
// Measured numbers and the steps that led here: DESIGN.md section 4.6.
#include "hpr.h"
#include "../../include/genpc_hip.h"

using namespace genpc;

// the call as asked: its sizes, the device's CU count (cus > 0: that count instead) and the switches
static HprAsk hpr_ask(int c, int n, int best_only, int cus)
{
    HprAsk a;
    a.c = c;
    a.n = n;
    a.best_only = best_only;
    a.cus = cus > 0 ? cus : num_cus();
    static const int env_split = tune_env("GENPC_HPR_SPLIT", -1, "hidden-point removal: 1 two-kernel form (first kernel stops after the home tiles, a wave per point continues), 0 one kernel, -1 pick by size");
    static const int no_cull = tune_env("GENPC_HPR_NOCULL", 0, "hidden-point removal: mask of alternative paths (128 no decisions without the walk in the wave-per-point pass, 512 two-kernel form WITH the first kernel's own verify phase)");
    static const int env_park = tune_env("GENPC_HPR_PARK_MB", 3072, "hidden-point removal, two-kernel form: MiB of polygon store (160 bytes per parked point; points beyond it restart in the wave-per-point pass)");
    static const int env_ht = tune_env("GENPC_HPR_HOME_TILES", 1, "hidden-point removal, two-kernel form: home tiles (1..3) the first kernel clips by before it parks a point");
    static const int env_hc = tune_env("GENPC_HPR_HOME_CHUNKS", 2, "hidden-point removal, two-kernel form with one home tile: 32-candidate chunks of it (1..4) the first kernel clips by");
    static const int env_dk = tune_env("GENPC_HPR_DECIDE_KERNEL", 1, "hidden-point removal: 1 = the parked points' first try in a kernel of its own (more waves per CU), 0 = inside the wave-per-point kernel");
    a.env_split = env_split;
    a.no_cull = no_cull;
    a.env_park_mb = env_park;
    a.env_home_tiles = env_ht;
    a.env_home_chunks = env_hc;
    a.env_decide_kernel = env_dk;
    return a;
}

static int hpr_run(int c, int n, const float *points, const double *eyes, double radius, unsigned char *visible, int *counts,
                   int *second_pass_points, void *stream_, int best_only, unsigned char *exact)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (c < 0 || n < 0 || !(radius > 0.0)) {
        set_error("genpc_hpr_visibility: bad size or radius");
        return -1;
    }
    if (second_pass_points) *second_pass_points = 0;
    if (c == 0) return 1;
    if (!counts || (n > 0 && (!points || !eyes || !visible))) {
        set_error("genpc_hpr_visibility: null pointer");
        return -1;
    }
    const HprAsk ask = hpr_ask(c, n, best_only, 0);
    const HprPlan plan = hpr_plan(ask);
    if (plan.too_large) {
        set_error("genpc_hpr_visibility: views x points too large (at most 4096 views per call)");
        return -1;
    }
    if (!check(hipMemsetAsync(counts, 0, sizeof(int) * (size_t)c, stream), "hipMemsetAsync(hpr counts)")) return 0;
    if (n == 0) return 1;
    HprCall k = {};
    k.c = c; k.n = n; k.points = points; k.eyes = eyes; k.radius = radius; k.visible = visible; k.counts = counts; k.no_cull = ask.no_cull;
    if (!hpr_sort_bytes((size_t)plan.pairs, stream, k.sort_bytes)) return 0;
    int *und; unsigned char *alive;
    WsLayout L;
    L.add(k.status, kHprStatusWords);          // the 256-byte header (hpr.h: HprStatus)
    L.add(k.fl, plan.fl_count);
    L.add(k.list, plan.pairs);
    L.add(k.k0, plan.pairs);
    L.add(k.k1, plan.pairs);
    L.add(k.i0, plan.pairs);
    L.add(k.i1, plan.pairs);
    L.add(k.sort_tmp, k.sort_bytes);
    L.add(k.tiles, plan.tile_count);
    L.add(k.hard, plan.pairs);
    L.add(k.hardlist, plan.pairs);
    L.add(k.hardcnt, c);
    L.add(und, c);
    L.add(alive, c);
    L.add(k.dup, n);
    L.add(k.work, kHprWorkWords);          // hpr.h: HprWork
    L.add(k.surv, plan.surv_count);
    if (!ws_alloc(L, kWsHpr, stream)) return 0;
    // views are dropped only when the plan says so: the passes see null otherwise
    k.und = plan.prune ? und : nullptr;
    k.alive = plan.prune ? alive : nullptr;
    // (the parked points' polygons and the global tier's buffers: workspaces of their own)
    if (plan.split && !(k.surv_poly = (double2 *)workspace(kWsHprParked, (size_t)plan.park_bytes, stream))) return 0;
    if (!(k.gbuf = (double2 *)workspace(kWsHprGlobalPolys, (size_t)plan.global_bytes, stream))) return 0;
    if (!check(hipMemsetAsync(k.status, 0, kHprStatusWords * sizeof(int), stream), "hipMemsetAsync(hpr status)")) return 0;
    if (!check(hipMemsetAsync(k.bounds(), 0xff, 12, stream), "hipMemsetAsync(hpr bounds)")) return 0;
    if (!hpr_launch_order(plan, k, stream) || !hpr_launch_accept(plan, k, stream) || !hpr_launch_first(plan, k, stream) ||
        !hpr_launch_wave(plan, k, stream))
        return 0;
    // the counters are fetched (the entry's only stream synchronisation) when somebody asks for them
    if (second_pass_points) {
        int st[kHprStBounds] = {0};
        if (!check(hipMemcpyAsync(st, k.status, sizeof st, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(hpr status)")) return 0;
        if (!check(hipStreamSynchronize(stream), "hipStreamSynchronize(hpr)")) return 0;
        *second_pass_points = st[kHprStListed] + st[kHprStParked];      // every point a wave took over (parked or listed)
        if (st[kHprStError]) {
            set_error("genpc_hpr_visibility: internal error (a normal-cone polygon outgrew its buffer)");
            return 0;
        }
    }
    if (exact) {
        if (plan.prune) {
            if (!check(hipMemcpyAsync(exact, k.alive, (size_t)c, hipMemcpyDeviceToDevice, stream), "hipMemcpyAsync(hpr exact)")) return 0;
        } else if (!check(hipMemsetAsync(exact, 1, (size_t)c, stream), "hipMemsetAsync(hpr exact)")) return 0;
    }
    return 1;
}

#ifdef GENPC_HPR_PROF
extern "C" __attribute__((visibility("default"))) int genpc_hpr_prof_read(unsigned long long *out, int reset)
{
    unsigned long long first[16], wave[16];
    if (!hpr_first_prof_read(first, reset) || !hpr_wave_prof_read(wave, reset)) return 0;
    for (int i = 0; i < 16; i++) out[i] = first[i] + wave[i];          // (the first pass writes slots 0 .. 8, the walk 9 .. 15)
    return 1;
}
#endif

GENPC_API int genpc_hpr_visibility(int c, int n, const float *points, const double *eyes, double radius, unsigned char *visible,
                                   int *counts, int *second_pass_points, void *stream_)
{
    return hpr_run(c, n, points, eyes, radius, visible, counts, second_pass_points, stream_, 0, nullptr);
}

GENPC_API int genpc_hpr_best_view_counts(int c, int n, const float *points, const double *eyes, double radius,
                                         unsigned char *visible, int *counts, unsigned char *exact, int *second_pass_points,
                                         void *stream_)
{
    return hpr_run(c, n, points, eyes, radius, visible, counts, second_pass_points, stream_, 1, exact);
}

GENPC_API int genpc_hpr_plan(int c, int n, int best_only, int cus, int out[24])
{
    if (!out || c < 0 || n < 0) return -1;
    const HprAsk ask = hpr_ask(c, n, best_only, cus);
    const HprPlan p = hpr_plan(ask);
    const int v[24] = {p.too_large, p.ntiles, p.split, p.prune, p.key_bits, p.max_clips, p.home_tiles, p.home_chunks, p.chunk_w, p.straggle_from,
                       p.straggle_lanes, (int)p.park_cap, p.decide_kernel, p.row_grid, p.bounds_grid, p.view_grid, p.decide_blocks, p.walk_blocks,
                       p.large_blocks, p.global_blocks, p.gcap, (int)(p.park_bytes >> 20), (int)(p.global_bytes >> 20), ask.cus};
    for (int i = 0; i < 24; i++) out[i] = v[i];
    return 1;
}
