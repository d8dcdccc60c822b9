// pose_plan.h -- the shape of one alignment call (pose.hip genpc_pose_optimize_batch) and of one silhouette step
// (mask_loss.hip mask_step), decided from values alone: which launches there are, on how many streams, how they hand over,
// how wide they are.  The loop and mask_step branch on nothing but what these two functions return.
// Host code only, no HIP: a plain C++ program can include it (tests/pose_plan_check.cpp does, with every threshold below
// as a row of its table).
#pragma once
#include <algorithm>

namespace genpc {

constexpr int kQBlock = 256;       // threads per block of the loop's point kernels (pose.h, mask.h: their launch bound)
// the reference's camera (diff_obj_pose.py:108-134): here because mask_step_plan sizes a disc with it; mask.h has the renderer's rest
constexpr float kMaskFocal = 4.0f, kMaskEyeZ = 3.0f, kMaskZnear = 1e-4f, kMaskZfar = 5.0f;

// blocks of kQBlock threads over n items, at most 1024 per row
inline int lin_grid(long long n)
{
    long long g = (n + kQBlock - 1) / kQBlock;
    if (g > 1024) g = 1024;
    if (g < 1) g = 1;
    return (int)g;
}

// Everything the decisions depend on, as values.
struct PoseLoopAsk {
    int scans = 1, starts = 1, nc = 0, np = 0;      // the call: b, starts, points of the complete / partial cloud
    bool mask = false;                              // the full objective (mask_weight != 0)
    int t_pose_dual = -1, t_pose_seeded = -1;       // the calling thread's modes (genpc_pose_dual, genpc_pose_tune); -1 = unset
    // the six GENPC_POSE_* switches (tune_env in pose.hip), at their defaults
    int env_lock = 1, env_seeded = 2, env_dual = 1, env_fuse_upd = 1, env_dual_flags = 1, env_ride = 1;
    bool side_stream_ok = true;                     // pose_side_of delivered a side stream with its events
    bool counters_ok = true;                        // ... and its device counters
    bool serialised_tool = false;                   // a tool runs one kernel at a time (ROCPROF_COUNTER_COLLECTION, AMD_SERIALIZE_KERNEL)
};

// Everything the loop then reads.
struct PoseLoopPlan {
    int lock;             // > 0: the starts of a scan side by side as batch elements (element = scan * lock + start)
    int elements;         // batch elements per launch
    int starts_left;      // passes of iters + 1 steps
    bool wants_side;      // the WISH for a side stream (the parent's dual_small): asked before there is one, see pose_wants_side
    bool dual;            // the Chamfer half of a step on the side stream
    bool flags;           // the two streams hand over through device counters (otherwise: events)
    bool fuse_upd;        // the Adam update of a step inside the next step's transform launch
    bool ride;            // pose_grad's blocks in mask_grad's launch
    int seed_mode;        // nearest neighbours from the second step on: 0 brute-force filter, 1 seeded cell search, 2 measure both and switch
    int g_t, g_g, gb;     // blocks per element of the transform, of pose_grad; blocks of the one-thread-per-element kernels
};

// The multi-starts of a scan are independent optimisations of the same clouds (diff_obj_pose.py:516-576): they run
// SIDE BY SIDE as batch elements (element = scan * starts + start) -- one pass of iters + 1 Adam steps with
// `starts` times the work per launch instead of `starts` passes.  At the reference's sizes every kernel of a
// step is latency-bound (15403 x 7855 points: 118 us of kernels per step, 804 steps = 95 ms of reg()'s 110),
// so the wider launches are nearly free.  Same arithmetic per element, same selection rule at the end.
inline int pose_lock(const PoseLoopAsk &a)
{
    return (a.starts > 1 && a.env_lock && (long long)a.scans * a.starts <= 256) ? a.starts : 0;
}

// Whether the call wishes for a side stream.  The loop asks this first and only then asks pose_side_of for one (a call that
// does not want a side stream makes none); what came back goes into side_stream_ok / counters_ok.
// On by default for small clouds (GENPC_POSE_DUAL=0 / genpc_pose_dual(0): one stream).  The side stream is of the highest
// priority class: as a stream of the caller's class it could land on the main stream's hardware queue and run BEHIND it
// (tools/time_c2_streams.py, one scan at a time: 24.4 scans/s without a side stream; 25.7 with it on the null stream but 21.2
// on a stream of the caller's own; with its own class 25.3 / 25.9).
// Small clouds only -- up to 65536 points per call, elements x points: where the launches fill the chip by themselves the two
// halves only take each other's compute units (8 scans in lock-step 77.6 -> 53.2 scans/s).
inline bool pose_wants_side(const PoseLoopAsk &a)
{
    const int lock = pose_lock(a);
    const long long elements = lock ? (long long)a.scans * lock : a.scans;
    return a.mask && (a.t_pose_dual >= 0 ? a.t_pose_dual != 0 : a.env_dual != 0) && elements * a.nc <= 65536;
}

inline PoseLoopPlan pose_loop_plan(const PoseLoopAsk &a)
{
    PoseLoopPlan p{};
    p.lock = pose_lock(a);
    p.elements = p.lock ? a.scans * p.lock : a.scans;
    p.starts_left = p.lock ? 1 : a.starts;
    const int b = p.elements;
    p.wants_side = pose_wants_side(a);
    p.dual = p.wants_side && a.side_stream_ok;

    // genpc_pose_tune(1) / GENPC_POSE_SEEDED=1 (the default is 2 = adaptive): from the second step on every nearest-neighbour
    // query starts from the index it was answered with a step ago and searches only the ball that answer leaves
    // (nn_seeded.hip): both clouds sorted once per call into uniform grids, the moving one in its rest frame.  Bit-identical
    // to the brute-force filter.
    // Measured (round 4): 8 scans of uniform VOLUME clouds 161 -> 120 ms per call (49 -> 66 scans/s: a rotated cube is still
    // a cube, every query keeps a near target), one scan 33.7 -> 32.2 ms (at that size a step is eight dependent launches,
    // not their work) -- but config 5's surfaces 0.67 -> 0.84 s: three of the four starts are rotated by 90 / 180 / 270
    // degrees, most queries of a misaligned start have NO near target, and the ball their old answer leaves crosses the
    // other surface over hundreds of cells (18 k instructions per wave, 4.8 ms per step against 3.0 for the filter, which
    // does not care where the points are).  Real shapes look like config 5: mode 1 is off by default.
    // (the grids hold clouds of 256 points and more)
    p.seed_mode = a.nc >= 256 && a.np >= 256 ? (a.t_pose_seeded >= 0 ? a.t_pose_seeded : a.env_seeded) : 0;
    // The two size gates below apply only while t_pose_seeded < 0: a thread that asks for 1 or 2 gets it at any size with
    // nc, np >= 256.
    // Small clouds with the full objective: the nearest-neighbour launches run on the side stream beside the silhouette half
    // and are not what a step waits for -- the adaptive mode's timing probes, ~10 host synchronisations per call, would cost
    // more than either choice: the filter it is.
    // (wants_side, the WISH for a side stream, switches the adaptive search off -- not `dual`, which is whether pose_side_of
    //  delivered one: a call that wished and got none still runs the filter.)
    if (p.wants_side && a.t_pose_seeded < 0 && p.seed_mode == 2) p.seed_mode = 0;
    // ... and so it is for small clouds in general: at the post-voxel sizes of reg() (4 x 4493 against 886 points) a step's
    // nearest-neighbour launches are ~17 us whichever way (the seeded search forced: 20.3 scans/s against 24.5), the adaptive
    // mode's ten timing probes each drain the stream (~40 us of nothing enqueued)
    if (a.t_pose_seeded < 0 && p.seed_mode == 2 && (long long)b * a.nc <= 24576) p.seed_mode = 0;

    // (measured: 4 elements 25.0 -> 26.1 completed scans/s, 32 elements 75.0 -> 74.1: every block repeats the update)
    p.fuse_upd = a.mask && a.env_fuse_upd != 0 && b <= 8;
    // The two streams of a step hand over through DEVICE WORDS, not events (round 6): an event record between the transform and
    // the splat and an event wait in front of the next transform each put ~3 us of command-processor latency on the step's critical
    // path (14.1 -> 12.2 ms per 201 steps without them, measured with the ordering switched off).  It is the fused update that
    // waits for pose_grad's count, so no counters without it.
    // (not under tools that run one kernel at a time -- rocprofv3's counter collection, AMD_SERIALIZE_KERNEL: a kernel that waits for
    //  a count can then sit in front of the kernel that publishes it, until its spin gives up; the events order the launches instead)
    p.flags = p.dual && p.fuse_upd && a.env_dual_flags != 0 && a.counters_ok && !a.serialised_tool;
    // one stream and the full objective: pose_grad's blocks ride at the end of the silhouette gradient's launch
    p.ride = a.mask && !p.dual && a.env_ride != 0;

    // (every block of the gradient kernels ends in 13-22 double atomics on its image's accumulators: with many images in
    // flight fewer, longer blocks per image)
    // 32 images (8 scans x 4 starts): 96 blocks per image 153.1 ms per call, 48: 151.0, 24: 150.2, 12: 150.4
    p.g_t = lin_grid(a.nc);
    p.g_g = std::min(b >= 16 ? 24 : 1024, lin_grid((long long)a.nc + a.np));
    p.gb = (b + 63) / 64;
    return p;
}

// One silhouette step of `elements` images of S x S pixels, nc points each drawn with `radius` (mask_step).
struct MaskStepPlan {
    int gp;            // blocks per image of the per-pixel launches
    int gs;            // blocks per image of mask_sums_kernel
    bool fuse_w;       // the per-pixel weights evaluated inside the gather instead of by mask_w_kernel
    bool sub8;         // eight lanes per point in mask_grad_kernel (otherwise one)
};

inline MaskStepPlan mask_step_plan(int elements, int nc, int S, float radius)
{
    MaskStepPlan p{};
    const float rad = 1.1f * radius;      // diff_obj_pose.py:385: the posed cloud is drawn with 1.1 x the radius
    p.gp = lin_grid((long long)S * S);
    // few blocks per image: every block ends in 22 double atomics on the image's accumulators, and 196 blocks x 22 on the
    // same addresses serialise in L2 (17.5 us for 0.2 M pixels)
    p.gs = std::min(p.gp, 48);      // 196: 221 ms per 8-scan call, 48: 210, 24: 210, 12: 210 (single scan: 42.1 / 41.4 / 41.8 / 43.3)
    // the weights per pixel as a launch of their own, or evaluated inside the gather
    // (only where the gather touches fewer pixels than ~three and a half passes over the image (config 2: 4493 points): a point's disc covers ~pi rho^2 pixels, rho =
    //  S/2 * focal * radius / 3 at the camera's distance -- 2451 points: 0.4 of the image; 16384 points: 2.9 images' worth of
    //  weights, each 60 instructions where the launch of its own computes them once per pixel)
    const float rho_px = 0.5f * (float)S * kMaskFocal * rad / kMaskEyeZ;
    p.fuse_w = (double)nc * 3.1416 * rho_px * rho_px <= 3.5 * (double)S * S;
    // lanes per point: a thread per point walks its whole pixel box alone (a chain of ~35 dependent gathers at the loop's
    // radius: 21 us for 4 x 2451 points), eight lanes share it row by row (12.9 us) -- until the points fill the chip by
    // themselves (measured at 4 x 16384 points, the four starts in lock-step: <1> 35 us, <8> 42)
    p.sub8 = (long long)elements * nc <= 24576 || elements <= 2;
    return p;
}

}  // namespace genpc
