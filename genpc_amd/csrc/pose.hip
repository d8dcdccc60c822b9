// pose.hip -- the SE(3)+scale alignment loop of optim_registration/diff_obj_pose.py
//  for gfx950: 7-DoF pose model (6D rotation, translation,
// log-scale), both halves of compute_loss_function (Chamfer, and the silhouette terms on an
// own differentiable occupancy splat -- the reference's Pulsar renderer is absent and
// unpinned, see mask_render.hip; the loss on its images is mask_loss.hip's), analytic backward, Adam.
// This file: the pose kernels, the entry points and the loop.  What the three files share of device code is pose.h and mask.h;
// what shape a call takes -- streams, hand-over, fused launches, grid sizes -- is decided in pose_plan.h, from values alone.
//
// The reference runs this through torch autograd: per iteration ~40 tiny kernels,
// two chamfer_3DDist calls (each computing BOTH directions and dropping one,
// utils/loss_util.py:35-38), two backward launches with 6 atomics per point, and a
// host round trip for the tqdm postfix.  Here an iteration of the Chamfer-only objective is four launches with no
// host synchronisation (the full objective adds the silhouette half -- mask_step, mask_loss.hip -- and, since round 6, folds the
// update into the next iteration's transform and runs the two halves on two streams that hand over through device
// counters: see PoseFuse and pose_publish_block in pose.h):
//   pose_transform_kernel   pts = (R ((v - c) s)^T)^T + c + t
//   nn_forward_kernel       ONE bidirectional NN (chamfer.hip): d1/i1 and d2/i2 are
//                           exactly the two partial-matching terms
//   pose_grad_kernel        d loss / d (R, s, t) reduced straight from (d, idx): the
//                           per-point gradient is never materialised, no atomics on
//                           point buffers; fp64 block reduction, one fp64 atomic per
//                           block and quantity
//   pose_update_kernel      (one wave) orthogonality term, 6D Gram-Schmidt backward,
//                           Adam for the three parameter groups, loss history,
//                           best-of-starts bookkeeping
// S scans of DIFFERENT sizes run through the same kernels in one call (genpc_pose_optimize_ragged, at the end of this file): every
// per-point kernel takes an optional element table (pose.h pose_span), the call's shape is pose_ragged_plan.h's -- one stream, the
// update a launch of its own, nearest neighbours from nn_ragged.hip's grid search or, on request, nn_ragged_dense.hip's all-pairs
// search -- and its two own kernels are pose_ragged.hip's.
// HBM traffic per iteration is O(N): ~24 B/point for the transform, ~28 B/point for
// the gradient pass; the NN launch dominates (VALU-bound, see chamfer.hip).
#include "nn.h"
#include "mask.h"
#include "fps.h"
#include "pose_ragged_plan.h"
#include "../../include/genpc_hip.h"

#include <math.h>
#include <stdlib.h>
#include <map>
#include <mutex>
#include <utility>

// chamfer.hip
extern "C" int genpc_chamfer_forward(int b, int n, const float *xyz1, int m, const float *xyz2, float *dist1,
                                     int *idx1, float *dist2, int *idx2, void *stream);

namespace genpc {

int genpc_mean3(int b, int n, const float *v, float *out, double *accum, hipStream_t st, const int *off = nullptr);

// diff_obj_pose.py:419-423
// blockIdx.y = batch element; element e reads v + e*n*3, center + e*cstride,
// params + e*pstride (strides in floats) and writes pts + e*n*3.
__global__ __launch_bounds__(kQBlock) void pose_transform_kernel(int n, const float *__restrict__ v,
                                                                 const float *__restrict__ center, int cstride,
                                                                 const float *__restrict__ params, int pstride,
                                                                 float *__restrict__ pts, const int *__restrict__ off = nullptr)
{
    const int e = blockIdx.y;
    const PoseSpan sp = pose_span(off, e, n);
    n = sp.n;
    v += sp.base * 3;
    pts += sp.base * 3;
    center += (size_t)e * cstride;
    params += (size_t)e * pstride;
    float R[9];
    rot6d_to_matrix(params, R);
    const float s = expf(params[9]);
    const float c[3] = {center[0], center[1], center[2]};
    const float t[3] = {params[6], params[7], params[8]};
    for (int j = blockIdx.x * kQBlock + threadIdx.x; j < n; j += gridDim.x * kQBlock) {
        float o[3];
        pose_point(R, s, c, t, v[(size_t)j * 3 + 0], v[(size_t)j * 3 + 1], v[(size_t)j * 3 + 2], o);
        pts[(size_t)j * 3 + 0] = o[0];
        pts[(size_t)j * 3 + 1] = o[1];
        pts[(size_t)j * 3 + 2] = o[2];
    }
}

__global__ void pose_wait_kernel(unsigned *ctr, int which, unsigned target)
{
    if (threadIdx.x == 0) (void)pose_wait_count(ctr, which, target);
}

__global__ __launch_bounds__(kQBlock) void pose_grad_kernel(int nc, const float *__restrict__ v,
                                                            const float *__restrict__ center, int cstride,
                                                            const float *__restrict__ params, int pstride, int np,
                                                            const float *__restrict__ partial,
                                                            const float *__restrict__ d1, const int *__restrict__ i1,
                                                            const float *__restrict__ d2, const int *__restrict__ i2,
                                                            float cd_weight, double *__restrict__ accum, unsigned *ctr,
                                                            const int *__restrict__ coff = nullptr, const int *__restrict__ poff = nullptr)
{
    __shared__ double red[15][kQBlock / kWave];
    pose_grad_body(blockIdx.x, gridDim.x, blockIdx.y, nc, v, center, cstride, params, pstride, np, partial, d1, i1, d2, i2, cd_weight, accum, red,
                   coff, poff);
    if (ctr) pose_publish_block(ctr, 1);
}

__global__ void pose_update_kernel(int b, PoseState *__restrict__ S, double *__restrict__ accum, int nc, int np,
                                   float cd_weight, float reg_weight, float lr, int do_step,
                                   float *__restrict__ history_slot, int history_stride,
                                   const int *__restrict__ coff = nullptr, const int *__restrict__ poff = nullptr)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= b) return;
    nc = pose_span(coff, e, nc).n;
    np = pose_span(poff, e, np).n;
    pose_update_one(S + e, accum + (size_t)e * kAcc, nc, np, cd_weight, reg_weight, lr, do_step,
                    history_slot ? history_slot + (size_t)e * history_stride : (float *)nullptr, true);
}

// start < 0: global init.  Otherwise begin start `start` (get_init_rot('y', 90*start),
// trans 0, log_scale log(0.75): diff_obj_pose.py:367,519).
// start_mod > 0: the starts of a scan run side by side (element e = scan * start_mod + start): start = e % start_mod.
__global__ void pose_begin_kernel(int b, PoseState *__restrict__ S, double *__restrict__ accum, int start, int start_mod)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= b) return;
    if (start >= 0 && start_mod > 0) start = e % start_mod;
    S += e;
    accum += (size_t)e * kAcc;
    if (start < 0) {
        S->best_loss = __builtin_inff();
        for (int k = 0; k < 10; k++) S->best_params[k] = 0.0f;
        for (int k = 0; k < kAcc; k++) accum[k] = 0.0;
        return;
    }
    const double th = start * 90.0 * M_PI / 180.0;
    const float init[10] = {(float)cos(th), 0.0f, (float)sin(th), 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, logf(0.75f)};
    for (int k = 0; k < 10; k++) {
        S->params[k] = init[k];
        S->m[k] = 0.0f;
        S->v[k] = 0.0f;
    }
    S->local_best = __builtin_inff();
    S->step = 0;
    S->patience_counter = 0;
    S->stopped = 0;
}

// What a call returns for one scan: the parameters p themselves, where asked for, and T = [[sR, t],[0,1]] (diff_obj_pose.py:464-468)
__device__ __forceinline__ void pose_emit(const float *p, float *T, float *params_out)
{
    if (params_out)
        for (int k = 0; k < 10; k++) params_out[k] = p[k];
    float R[9];
    rot6d_to_matrix(p, R);
    const float s = expf(p[9]);
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) T[a * 4 + b] = R[a * 3 + b] * s;
        T[a * 4 + 3] = p[6 + a];
    }
    T[12] = T[13] = T[14] = 0.0f;
    T[15] = 1.0f;
}

// end of a start: keep the FINAL parameters of the start with the lowest loss seen
// (diff_obj_pose.py:570-576).  final != 0: also emit T and the parameters (pose_emit).
__global__ void pose_end_kernel(int b, PoseState *__restrict__ S, int final, float *__restrict__ transform,
                                float *__restrict__ best_params)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= b) return;
    S += e;
    if (transform) transform += (size_t)e * 16;
    if (best_params) best_params += (size_t)e * 10;
    if (!final) {
        if (S->local_best < S->best_loss) {
            S->best_loss = S->local_best;
            for (int k = 0; k < 10; k++) S->best_params[k] = S->params[k];
        }
        return;
    }
    pose_emit(S->best_params, transform, best_params);
}

// Lock-step starts: the `starts` elements of scan g have finished side by side; apply the sequential rule of
// diff_obj_pose.py:570-576 in start order (strict <: the first of equal lowest losses wins) and emit that start's
// FINAL parameters and T = [[sR, t],[0,1]].
__global__ void pose_pick_kernel(int scans, int starts, const PoseState *__restrict__ S, float *__restrict__ transform,
                                 float *__restrict__ best_params)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= scans) return;
    float best_loss = __builtin_inff();
    int best = 0;
    for (int s = 0; s < starts; s++) {
        const float l = S[g * starts + s].local_best;
        if (l < best_loss) { best_loss = l; best = s; }
    }
    pose_emit(S[g * starts + best].params, transform + (size_t)g * 16, best_params ? best_params + (size_t)g * 10 : (float *)nullptr);
}

// dst[g, r, :] = src[g, :] for r < rep (count floats per row)
__global__ __launch_bounds__(kQBlock) void pose_replicate_kernel(size_t count, int rep, const float *__restrict__ src,
                                                                 float *__restrict__ dst)
{
    const int g = blockIdx.y;
    for (size_t j = (size_t)blockIdx.x * kQBlock + threadIdx.x; j < count; j += (size_t)gridDim.x * kQBlock) {
        const float v = src[(size_t)g * count + j];
        for (int r = 0; r < rep; r++) dst[((size_t)g * rep + r) * count + j] = v;
    }
}

// pose_transform_kernel and mask_project_kernel (posed) in one launch: both walk the complete cloud with the same
// parameters (one 5 us launch less per Adam step; the same arithmetic, so the same bits in pts and uvr)
__global__ __launch_bounds__(kQBlock) void pose_transform_project_kernel(int n, const float *__restrict__ v,
                                                                         const float *__restrict__ center, int cstride,
                                                                         const float *__restrict__ params, int pstride,
                                                                         float *__restrict__ pts, float radius, int S,
                                                                         float4 *__restrict__ uvr, int *__restrict__ bins,
                                                                         float *__restrict__ zex, PoseFuse fu,
                                                                         const int *__restrict__ off = nullptr)
{
    __shared__ float s_par[10];
    const int e = blockIdx.y;
    const PoseSpan sp = pose_span(off, e, n);
    n = sp.n;
    v += sp.base * 3;
    pts += sp.base * 3;
    uvr += sp.base;
    if (zex) zex += sp.base;
    int *bin_cnt = bins ? bins + (size_t)e * bins_tiles(S) : nullptr;
    int *bin_idx = bins ? bins + (size_t)gridDim.y * bins_tiles(S) + (size_t)e * bins_tiles(S) * kTileCap : nullptr;
    center += (size_t)e * cstride;
    params = pose_fused_params(fu, e, params + (size_t)e * pstride, s_par);      // (the previous step's update, when fused)
    float R[9];
    rot6d_to_matrix(params, R);
    const float s = expf(params[9]);
    const float c[3] = {center[0], center[1], center[2]};
    const float t[3] = {params[6], params[7], params[8]};
    const float hs = 0.5f * S;
    __shared__ int s_cnt[kBinTiles], s_base[kBinTiles];
    for (int j0 = blockIdx.x * kQBlock; j0 < n; j0 += gridDim.x * kQBlock) {        // (block-uniform: bin_points_block has barriers)
        const int j = j0 + threadIdx.x;
        const bool valid = j < n;
        const int jj = valid ? j : n - 1;
        float o[3];
        pose_point(R, s, c, t, v[(size_t)jj * 3 + 0], v[(size_t)jj * 3 + 1], v[(size_t)jj * 3 + 2], o);
        const SplatPt q = splat_project(o, radius, hs);
        if (valid) {
            pts[(size_t)j * 3 + 0] = o[0];
            pts[(size_t)j * 3 + 1] = o[1];
            pts[(size_t)j * 3 + 2] = o[2];
            uvr[j] = make_float4(q.u, q.v, q.ok ? q.rho : -1.0f, q.ok ? 1.0f / (q.rho * q.rho) : 0.0f);
            if (zex) zex[j] = pulsar_ze(q.zv);
        }
        if (bin_cnt) bin_points_block(bin_cnt, bin_idx, s_cnt, s_base, S, valid && q.ok, j, q.u, q.v, q.rho);
    }
    if (fu.ctr) pose_publish_block(fu.ctr, 0);
}

}  // namespace genpc

GENPC_API int genpc_pose_transform(int n, const float *v, const float *center, const float *params, float *pts,
                                   void *stream)
{
    using namespace genpc;
    if (n <= 0) return 1;
    hipLaunchKernelGGL(pose_transform_kernel, dim3(lin_grid(n), 1), dim3(kQBlock), 0, (hipStream_t)stream, n, v, center,
                       0, params, 0, pts);
    return check(hipGetLastError(), "pose_transform launch") ? 1 : 0;
}

GENPC_API int genpc_pose_loss_grad(int nc, const float *v, const float *vert_col, const float *center, const float *params,
                                   int np, const float *partial, const float *partial_col, const float *d1, const int *i1,
                                   const float *d2, const int *i2, float cd_weight, float reg_weight, float mask_weight,
                                   float radius, int render_size, float *loss_out, float *grad, void *stream)
{
    using namespace genpc;
    if (nc <= 0 || np <= 0) return -1;
    const bool mask = mask_weight != 0.0f;
    if (mask && (render_size <= 1 || !(radius > 0.0f))) return -1;
    hipStream_t st = (hipStream_t)stream;
    const size_t P = mask ? (size_t)render_size * render_size : 0;
    const size_t nmax = (size_t)(nc > np ? nc : np);
    double *accum; PoseState *S;
    MaskScratch m;
    WsLayout L;
    L.add(accum, 64);          // (kAcc sums in a 512-byte piece)
    L.add(S, 1);
    m.layout(L, 1, P, nmax);
    if (!ws_alloc(L, kWsPoseLossGrad, st)) return 0;
    if (P && !m.zero_bins(st)) return 0;
    if (!check(hipMemsetAsync(accum, 0, kAcc * sizeof(double), st), "hipMemsetAsync(accum)")) return 0;
    if (!check(hipMemcpyAsync(S->params, params, 10 * sizeof(float), hipMemcpyDeviceToDevice, st), "copy params"))
        return 0;
    hipLaunchKernelGGL(pose_grad_kernel, dim3(lin_grid((long long)nc + np), 1), dim3(kQBlock), 0, st, nc, v, center, 0,
                       params, 0, np, partial, d1, i1, d2, i2, cd_weight, accum, (unsigned *)nullptr);
    if (mask) {
        if (!mask_prepare_ref(1, np, partial, partial_col, radius, render_size, m, st)) return 0;
        if (!mask_step(1, nc, v, vert_col, center, 0, params, 0, radius, render_size, mask_weight, m, accum, st)) return 0;
    }
    hipLaunchKernelGGL(pose_update_kernel, dim3(1), dim3(64), 0, st, 1, S, accum, nc, np, cd_weight, reg_weight, 0.0f, 0,
                       (float *)nullptr, 0);
    if (!check(hipMemcpyAsync(grad, S->grad, 10 * sizeof(float), hipMemcpyDeviceToDevice, st), "copy grad")) return 0;
    if (!check(hipMemcpyAsync(loss_out, S->loss, 4 * sizeof(float), hipMemcpyDeviceToDevice, st), "copy loss")) return 0;
    return check(hipGetLastError(), "pose_loss_grad launch") ? 1 : 0;
}

GENPC_API int genpc_pose_cd_grad(int nc, const float *v, const float *center, const float *params, int np,
                                 const float *partial, const float *d1, const int *i1, const float *d2, const int *i2,
                                 float cd_weight, float reg_weight, float *loss_out, float *grad, void *stream)
{
    // loss_out[3]: total, cd, ortho (the Chamfer half alone)
    using namespace genpc;
    hipStream_t st = (hipStream_t)stream;
    float *tmp = (float *)workspace(kWsPoseCdLoss, 256, st);
    if (!tmp) return 0;
    const int rc = genpc_pose_loss_grad(nc, v, nullptr, center, params, np, partial, nullptr, d1, i1, d2, i2, cd_weight,
                                        reg_weight, 0.0f, 0.0f, 0, tmp, grad, stream);
    if (rc != 1) return rc;
    return check(hipMemcpyAsync(loss_out, tmp, 3 * sizeof(float), hipMemcpyDeviceToDevice, st), "copy loss") ? 1 : 0;
}

namespace genpc { thread_local int t_pose_seeded = -1; }

/* Nearest-neighbour path of the alignment loop, for tests and A/B (calling host thread): 1 seeded cell search from the
 * second step on (csrc/nn_seeded.hip: it wins when every query keeps a near target and loses on misaligned starts of
 * real shapes), 0 the brute-force filter at every step, 2 whichever of the two the call measures to be faster (the
 * default), < 0 the default / environment (GENPC_POSE_SEEDED).  All give the same bits for finite clouds (a NaN coordinate: the head of
 * nn_seeded.hip).  Returns the previous setting. */
GENPC_API int genpc_pose_tune(int seeded)
{
    const int prev = genpc::t_pose_seeded;
    genpc::t_pose_seeded = seeded < 0 ? -1 : (seeded > 2 ? 2 : seeded);
    return prev;
}

namespace genpc { static thread_local int t_pose_dual = -1; }

/* The calling host thread's alignment loops: 1 = the Chamfer half of a step on a side stream beside the silhouette half (small
 * clouds, full objective), 0 = one stream, < 0 = the default (GENPC_POSE_DUAL, on).  pipeline.run_in_lanes switches it off in
 * its lanes: with several scans in flight the chip is shared already and a second stream per scan costs throughput (six lanes:
 * 30 scans/s with, 40 without; one scan alone: 45.6 ms with, 48.3 without).  Returns the previous setting. */
GENPC_API int genpc_pose_dual(int on)
{
    const int prev = genpc::t_pose_dual;
    genpc::t_pose_dual = on < 0 ? -1 : (on ? 1 : 0);
    return prev;
}

namespace genpc {
// The two halves of an Adam step read the posed cloud and nothing of each other -- nearest neighbours + Chamfer gradient
// (three launches) and the silhouette term (splat, sums, gather) -- and every launch of either is latency-bound on a mostly
// idle chip: with the full objective the Chamfer half runs on a stream of its own beside the silhouette half (fork behind
// the transform, join in front of the update; all enqueued up front like the rest, no host synchronisation).  One side
// stream and a small ring of events per caller's stream, made once and kept for the life of the process.
struct PoseSide {
    hipStream_t side = nullptr;
    hipEvent_t fork[4] = {nullptr, nullptr, nullptr, nullptr}, join[4] = {nullptr, nullptr, nullptr, nullptr};
    bool ok = false;
    // hand-over through device words (pose_wait_count / pose_publish_block): counts that only grow, so nothing is reset between steps,
    // starts or calls; a call that returned early leaves `dirty` set and the next one starts from a synchronised, zeroed state
    unsigned *ctr = nullptr;
    unsigned tp_count = 0, pg_count = 0;
    bool dirty = false;
};
static PoseSide *pose_side_of(hipStream_t st)
{
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, PoseSide *> table;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> g(mu);
    auto it = table.find({dev, st});
    if (it != table.end()) return it->second->ok ? it->second : nullptr;
    PoseSide *p = new PoseSide();
    // (the highest priority class: streams of one class share a handful of hardware queues, and a side stream that lands on its
    //  main stream's queue runs behind it instead of beside it -- tools/time_c2_streams.py; the class's queues are its own)
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    p->ok = hipStreamCreateWithPriority(&p->side, hipStreamNonBlocking, prio_hi) == hipSuccess;
    for (int i = 0; i < 4 && p->ok; i++)
        p->ok = hipEventCreateWithFlags(&p->fork[i], hipEventDisableTiming) == hipSuccess &&
                hipEventCreateWithFlags(&p->join[i], hipEventDisableTiming) == hipSuccess;
    if (p->ok && (hipMalloc((void **)&p->ctr, 4 * sizeof(unsigned)) != hipSuccess || hipMemset(p->ctr, 0, 4 * sizeof(unsigned)) != hipSuccess))
        p->ctr = nullptr;          // (the events still work)
    table[{dev, st}] = p;
    return p->ok ? p : nullptr;
}

// The hand-over between the two streams of ONE call of the loop: where a step forks, counts and joins.  Without a side stream
// (side null) the nearest-neighbour launches go to the caller's stream and every method is a no-op.
// With `flags` the streams hand over through DEVICE WORDS, not events (why: pose_plan.h): the transform's blocks count
// themselves finished (release), a one-wave kernel on the side stream waits for that count in front of the Chamfer half;
// pose_grad's blocks count themselves, and thread 0 of every block of the NEXT transform waits for that count before it reads
// the sums (the fused update).  The last step of a start joins through an event as before (its update is a launch of its own).
struct PoseHandOver {
    PoseSide *side = nullptr;
    bool flags = false;
    hipStream_t st = nullptr, sn = nullptr;      // the caller's stream; the stream of the nearest-neighbour launches and pose_grad
    long long joins = 0;                         // (the events' ring index is joins & 3)

    // on the way in.  False: the repair of an earlier call's counts failed.
    bool begin(PoseSide *side_, bool flags_, hipStream_t st_)
    {
        side = side_; flags = flags_; st = st_;
        sn = side ? side->side : st;
        if (!flags) return true;
        if (side->dirty) {          // an earlier call left early: counts and expectations may disagree
            if (!check(hipStreamSynchronize(st), "hipStreamSynchronize") || !check(hipStreamSynchronize(side->side), "hipStreamSynchronize") ||
                !check(hipMemset(side->ctr, 0, 4 * sizeof(unsigned)), "hipMemset(counters)"))
                return false;
            side->tp_count = side->pg_count = 0;
        }
        side->dirty = true;
        return true;
    }
    unsigned *ctr() const { return flags ? side->ctr : (unsigned *)nullptr; }      // what the counted launches publish to
    unsigned grads_counted() const { return flags ? side->pg_count : 0u; }         // what the fused update waits for
    // behind the transform's launch of `blocks` blocks: the side stream's launches of this step wait for it
    void after_transform(unsigned blocks)
    {
        if (flags) {
            side->tp_count += blocks;
            hipLaunchKernelGGL(pose_wait_kernel, dim3(1), dim3(kWave), 0, sn, side->ctr, 0, side->tp_count);
        } else if (side) {
            (void)hipEventRecord(side->fork[joins & 3], st);
            (void)hipStreamWaitEvent(sn, side->fork[joins & 3], 0);
        }
    }
    // behind pose_grad's launch of `blocks` blocks (given ctr())
    void after_grad(unsigned blocks) { if (flags) side->pg_count += blocks; }
    // in front of an update that is a launch of its own: it reads both halves' sums
    void join(bool last_step)
    {
        if (side && (!flags || last_step)) {
            (void)hipEventRecord(side->join[joins & 3], sn);
            (void)hipStreamWaitEvent(st, side->join[joins & 3], 0);
            joins++;
        }
    }
    // on the way out, and only there: every launch of the call has been enqueued, counts and expectations agree
    void end() { if (flags) side->dirty = false; }
};

// Mode 2 of the loop's nearest-neighbour search (pose_plan.h seed_mode; modes 0 and 1 pass through with nothing timed).  What
// the seeded search costs depends on the data (a query whose last answer is far away searches a large ball: the hidden side of
// a complete shape against a one-sided scan; misaligned starts) and falls as the poses converge; the filter costs the same at
// every step.  Both give the same bits, so the choice is free: steps 0 and 2 time the filter (the first one carries the
// call's one-off costs: the smaller of the two counts), step 1 and then every probe_every-th time the seeded search, and the
// steps in between take whichever was faster last (two events and one wait per probe: ~10 per call).
struct PoseProbe {
    static constexpr int kPoseProbe = 25;
    // A probe of the seeded search while the filter is in use runs on every kPoseSample-th block only, in front of
    // the filter (which then answers the step, same bits): on a misaligned start of a real scan a full seeded step
    // costs a millisecond against the filter's 16 us, and three such probes were 5 % of a completed scan.
    static constexpr int kPoseSample = 4;
    struct Step {
        bool time_filter, time_seeded;      // this step is timed: the filter / the seeded search
        bool sampled;                       // ... the latter as a sampled launch in front of the filter
        bool run_seeded;                    // the seeded search answers the step (otherwise the filter)
        bool timed() const { return time_filter || time_seeded; }
    };
    int seed_mode = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float t_filter = 0.0f, t_seeded = __builtin_inff();
    bool use_seeded = false;
    int probe_every = kPoseProbe, next_probe = 1;          // (a probe that loses doubles the distance to the next one)

    // (the two events are released on EVERY way out of the loop's function, its early `return 0`s included: ADVICE r4)
    ~PoseProbe() { if (ev0) (void)hipEventDestroy(ev0); if (ev1) (void)hipEventDestroy(ev1); }
    bool init(int mode)
    {
        seed_mode = mode;
        use_seeded = mode == 1;
        if (mode == 2 && (hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess)) {
            set_error("pose_optimize: hipEventCreate failed");
            return false;
        }
        return true;
    }
    // (sequential starts: every start probes afresh)
    void arm()
    {
        if (seed_mode == 2) { probe_every = kPoseProbe; next_probe = 1; use_seeded = false; t_seeded = __builtin_inff(); }
    }
    Step step(int it) const
    {
        Step s;
        s.time_filter = seed_mode == 2 && (it == 0 || it == 2);
        s.time_seeded = seed_mode == 2 && it == next_probe && !s.time_filter;
        s.sampled = s.time_seeded && !use_seeded;
        s.run_seeded = seed_mode != 0 && it > 0 && !s.time_filter && use_seeded;
        return s;
    }
    // the three places of a timed step, on the stream of the nearest-neighbour launches: in front of them, behind a sampled
    // launch, behind them all (waits for the stream, reads the time and decides the steps to come)
    void before(const Step &s, hipStream_t sn) { if (s.timed()) (void)hipEventRecord(ev0, sn); }
    void sample_done(const Step &s, hipStream_t sn) { if (s.sampled) (void)hipEventRecord(ev1, sn); }
    void after(const Step &s, int it, hipStream_t sn)
    {
        float ms = 0.0f;
        if (!s.timed() || !((s.sampled || hipEventRecord(ev1, sn) == hipSuccess) && hipEventSynchronize(ev1) == hipSuccess &&
                            hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess))
            return;
        if (s.time_filter) {
            t_filter = it == 0 ? ms : (ms < t_filter ? ms : t_filter);
        } else {
            t_seeded = s.sampled ? ms * kPoseSample : ms;      // (a sample's launch overhead counts four times: errs towards the filter)
            const bool wins = t_seeded < 0.9f * t_filter;
            probe_every = wins ? kPoseProbe : 2 * probe_every;
            next_probe = it + probe_every;
        }
        // (the filter is the known quantity: the search must win clearly, and against a clean measurement)
        use_seeded = it >= 2 && t_seeded < 0.9f * t_filter;
    }
};

// Lock-step starts: every cloud of the call `rep` times in a row in scratch (element = scan * rep + start); the pointers move there
static bool pose_replicate(int scans, int rep, int nc, int np, const float *&complete, const float *&complete_col, const float *&partial,
                           const float *&partial_col, hipStream_t st)
{
    float *x_complete = nullptr, *x_partial = nullptr, *x_ccol = nullptr, *x_pcol = nullptr;
    const size_t xc = (size_t)scans * rep * nc * 3, xp = (size_t)scans * rep * np * 3;
    WsLayout X;          // (the colours' pieces are reserved whether or not the call brings colours)
    X.add(x_complete, xc);
    X.add(x_partial, xp);
    X.add(x_ccol, xc);
    X.add(x_pcol, xp);
    if (!ws_alloc(X, kWsPoseReplicas, st)) return false;
    hipLaunchKernelGGL(pose_replicate_kernel, dim3(lin_grid((long long)nc * 3), scans), dim3(kQBlock), 0, st, (size_t)nc * 3, rep, complete, x_complete);
    hipLaunchKernelGGL(pose_replicate_kernel, dim3(lin_grid((long long)np * 3), scans), dim3(kQBlock), 0, st, (size_t)np * 3, rep, partial, x_partial);
    if (complete_col)
        hipLaunchKernelGGL(pose_replicate_kernel, dim3(lin_grid((long long)nc * 3), scans), dim3(kQBlock), 0, st, (size_t)nc * 3, rep, complete_col, x_ccol);
    if (partial_col)
        hipLaunchKernelGGL(pose_replicate_kernel, dim3(lin_grid((long long)np * 3), scans), dim3(kQBlock), 0, st, (size_t)np * 3, rep, partial_col, x_pcol);
    complete = x_complete; partial = x_partial;
    complete_col = complete_col ? x_ccol : nullptr; partial_col = partial_col ? x_pcol : nullptr;
    return true;
}
}  // namespace genpc

/* The side streams the library pairs with `stream` (the alignment loop's second stream, the sampling check's), made NOW and
 * each given a first command, so that they get their hardware queues before the caller makes other streams: which queue
 * (and which of the command processor's pipes) a stream lands on is decided when it is first used, and a completed scan
 * whose side streams were first used after six lane streams existed ran at 26.7 scans/s against 28.9
 * (tools/c2_after_big.py).  pipeline.run_in_lanes calls it before it makes its lanes. */
GENPC_API int genpc_streams_prepare(void *stream)
{
    using namespace genpc;
    hipStream_t st = (hipStream_t)stream;
    PoseSide *p = pose_side_of(st);
    if (p) {
        (void)hipEventRecord(p->fork[0], p->side);
        (void)hipStreamSynchronize(p->side);
    }
    fps_deferred_prepare(st);
    return 1;
}

GENPC_API int genpc_pose_optimize_batch(int b, int nc, const float *complete, const float *complete_col, int np,
                                        const float *partial, const float *partial_col, float lr, int iters, int starts,
                                        float radius, int render_size, float mask_weight, float *transform,
                                        float *history, float *best_params, void *stream)
{
    using namespace genpc;
    if (b <= 0 || nc <= 0 || np <= 0 || iters < 0 || starts < 1) return -1;
    const bool mask = mask_weight != 0.0f;
    if (mask && (render_size <= 1 || !(radius > 0.0f))) return -1;
    hipStream_t st = (hipStream_t)stream;

    // The plan of the call (pose_plan.h: every decision and its reason) from the call, the thread's modes and the switches
    static const int env_lock = tune_env("GENPC_POSE_LOCKSTEP", 1, "alignment loop: 0 = the starts of a scan one after the other instead of side by side");
    static const int env_seeded = tune_env("GENPC_POSE_SEEDED", 2, "alignment loop, nearest neighbours from the second step on: 1 = seeded cell search, 0 = brute-force filter, 2 = measure both and switch");
    static const int env_dual0 = tune_env("GENPC_POSE_DUAL", 1, "alignment loop, full objective, small clouds: 1 = the Chamfer half of a step (nearest neighbours + gradient) on a side stream beside the silhouette half, 0 = one stream");
    static const int env_fuse_upd = tune_env("GENPC_POSE_FUSE_UPDATE", 1, "alignment loop, full objective: 1 = the Adam update of a step inside the next step's transform launch, 0 = a launch of its own");
    static const int env_dual_flags = tune_env("GENPC_POSE_DUAL_FLAGS", 1, "alignment loop with a side stream: 1 = the streams hand over through device counters, 0 = through events");
    static const int env_ride = tune_env("GENPC_POSE_GRAD_RIDES", 1, "alignment loop, one stream, full objective: 1 = pose_grad's blocks in mask_grad's launch, 0 = a launch of its own");
    static const bool serialised = [] {
        const char *a = getenv("ROCPROF_COUNTER_COLLECTION"), *b2 = getenv("AMD_SERIALIZE_KERNEL");
        return (a && *a && *a != '0') || (b2 && *b2 && *b2 != '0');
    }();
    PoseLoopAsk ask;
    ask.scans = b; ask.starts = starts; ask.nc = nc; ask.np = np; ask.mask = mask;
    ask.t_pose_dual = t_pose_dual; ask.t_pose_seeded = t_pose_seeded;
    ask.env_lock = env_lock; ask.env_seeded = env_seeded; ask.env_dual = env_dual0; ask.env_fuse_upd = env_fuse_upd;
    ask.env_dual_flags = env_dual_flags; ask.env_ride = env_ride;
    ask.serialised_tool = serialised;
    PoseSide *side = pose_wants_side(ask) ? pose_side_of(st) : nullptr;      // (a call that wants no side stream makes none)
    ask.side_stream_ok = side != nullptr;
    ask.counters_ok = side != nullptr && side->ctr != nullptr;
    const PoseLoopPlan plan = pose_loop_plan(ask);
    const int scans = b, starts_in = starts, gb = plan.gb;

    if (plan.lock && !pose_replicate(scans, plan.lock, nc, np, complete, complete_col, partial, partial_col, st)) return 0;
    b = plan.elements;
    starts = plan.starts_left;

    const size_t P = mask ? (size_t)render_size * render_size : 0;
    double *accum; PoseState *S; float *center, *pts, *d1, *d2; int *i1, *i2;
    MaskScratch m = {};
    WsLayout L;
    L.add(accum, (size_t)2 * b * kAcc);        // two sets: a step's sums are read by the next step's
    L.add(S, (size_t)2 * b);                   // transform (the fused update) while that step fills the other
    L.add(center, (size_t)b * 4);
    L.add(pts, (size_t)b * nc * 3);
    L.add(d1, (size_t)b * nc);
    L.add(d2, (size_t)b * np);
    L.add(i1, (size_t)b * nc);
    L.add(i2, (size_t)b * np);
    if (mask) m.layout(L, b, P, (size_t)(nc > np ? nc : np));
    if (!ws_alloc(L, kWsPoseLoop, st)) return 0;
    if (mask && !m.zero_bins(st)) return 0;
    constexpr int kStateFloats = (int)(sizeof(PoseState) / sizeof(float));
    static_assert(sizeof(PoseState) % sizeof(float) == 0, "PoseState must be float-addressable");
    PoseState *Sb[2] = {S, S + b};
    double *ab[2] = {accum, accum + (size_t)b * kAcc};

    // center = mean(vert_pos) per scan (diff_obj_pose.py:362)
    if (!genpc_mean3(b, nc, complete, center, accum, st)) return 0;
    if (!check(hipMemsetAsync(ab[1], 0, (size_t)b * kAcc * sizeof(double), st), "hipMemsetAsync(second accumulator set)")) return 0;
    // reference image of the partial cloud (render_reference_image, diff_obj_pose.py:108-134)
    if (mask && !mask_prepare_ref(b, np, partial, partial_col, radius, render_size, m, st)) return 0;
    // Exact duplicates (a partial cloud resampled with replacement, a crop pad-repeated to a fixed size) are the same
    // at every step -- the partial cloud does not move and equal rest-frame points are posed to equal points -- so
    // the filter's duplicate masks (nn_dedupe.hip) are made once per call, on the rest-frame clouds.
    const size_t w_p = (nn_dedupe_mask_words(b, np) + 63) & ~(size_t)63, w_c = (nn_dedupe_mask_words(b, nc) + 63) & ~(size_t)63;
    unsigned *dup_p = (unsigned *)workspace(kWsPoseDupMasks, (w_p + w_c) * sizeof(unsigned), st);
    if (!dup_p) return 0;
    unsigned *dup_c = dup_p + w_p;
    {
        const float *dp[2] = {partial, complete};
        const int dn[2] = {np, nc};
        unsigned *dm[2] = {dup_p, dup_c};
        if (!launch_nn_dedupe(b, 2, dp, dn, dm, nullptr, st)) return 0;
    }
    PoseProbe probe;
    if (!probe.init(plan.seed_mode)) return 0;
    SeededGrids sg{};
    if (plan.seed_mode != 0) {
        WsLayout GL;
        seeded_grids_layout(GL, sg, b, nc, np);
        if (!ws_alloc(GL, kWsPoseSeededGrids, st) || !build_seeded_grids(b, nc, complete, np, partial, sg, st)) return 0;
    }
    const int fma_mode = arith_mode() != 0 ? 1 : 0;

    hipLaunchKernelGGL(pose_begin_kernel, dim3(gb), dim3(64), 0, st, b, S, accum, -1, 0);
    const int hstride = starts * (iters + 1);
    PoseHandOver ho;
    if (!ho.begin(plan.dual ? side : nullptr, plan.flags, st)) return 0;
    hipStream_t sn = ho.sn;
    for (int s = 0; s < starts; s++) {
        probe.arm();
        hipLaunchKernelGGL(pose_begin_kernel, dim3(gb), dim3(64), 0, st, b, S, accum, s, plan.lock);
        for (int it = 0; it <= iters; it++) {
            // The update of step it - 1 rides in this step's transform (full objective; fuse_upd): state and accumulators ping-pong
            // between two sets -- this step's kernels read Sc and add into ac, the transform read the other set and zeroed ac.
            const int cur = plan.fuse_upd ? (it & 1) : 0;
            PoseState *Sc = Sb[cur];
            double *ac = ab[cur];
            float *hslot = history ? history + (size_t)s * (iters + 1) + it : (float *)nullptr;      // this step's loss, element 0
            // 1. transform
            if (mask) {
                PoseFuse fu{};
                if (plan.fuse_upd && it > 0) {
                    fu.S_in = Sb[cur ^ 1]; fu.S_out = Sc; fu.acc_in = ab[cur ^ 1]; fu.acc_zero = ac;
                    fu.do_update = 1; fu.nc = nc; fu.np = np; fu.lr = lr;
                    fu.history = hslot ? hslot - 1 : (float *)nullptr;
                    fu.hstride = hstride;
                    fu.pg_target = ho.grads_counted();
                }
                fu.ctr = ho.ctr();
                hipLaunchKernelGGL(pose_transform_project_kernel, dim3(plan.g_t, b), dim3(kQBlock), 0, st, nc, complete,
                                   (const float *)center, 4, (const float *)Sc->params, kStateFloats, pts, 1.1f * radius, render_size,
                                   m.uvr, use_bins(render_size) ? m.bins : (int *)nullptr, render_blend() ? m.zex : (float *)nullptr, fu);
            } else
                hipLaunchKernelGGL(pose_transform_kernel, dim3(plan.g_t, b), dim3(kQBlock), 0, st, nc, complete,
                                   (const float *)center, 4, (const float *)Sc->params, kStateFloats, pts);
            // 2. hand over to the side stream
            ho.after_transform((unsigned)plan.g_t * (unsigned)b);
            // 3. nearest neighbours, both directions
            const PoseProbe::Step ps = probe.step(it);
            probe.before(ps, sn);
            if (ps.sampled && launch_nn_seeded(b, nc, pts, np, partial, sg, center, 4, (const float *)Sc->params, kStateFloats, d1, i1, d2, i2,
                                               fma_mode, sn, PoseProbe::kPoseSample) != 1)
                return 0;
            probe.sample_done(ps, sn);
            if (ps.run_seeded) {
                if (launch_nn_seeded(b, nc, pts, np, partial, sg, center, 4, (const float *)Sc->params, kStateFloats, d1, i1, d2, i2, fma_mode, sn) != 1)
                    return 0;
            } else if (nn_forward(b, 2, pts, nc, partial, np, d1, i1, partial, np, pts, nc, d2, i2, sn, __builtin_inff(), dup_p, dup_c) != 1) {
                return 0;
            }
            probe.after(ps, it, sn);
            // 4. the Chamfer gradient: a launch of its own, or its blocks at the end of the silhouette gradient's launch
            PoseGradArgs pga{};
            if (plan.ride) {
                pga.nc = nc; pga.cstride = 4; pga.pstride = kStateFloats; pga.np = np;
                pga.v = complete; pga.center = center; pga.params = Sc->params; pga.partial = partial;
                pga.d1 = d1; pga.d2 = d2; pga.i1 = i1; pga.i2 = i2;
                pga.cd_weight = 3.0f; pga.accum = ac; pga.gx = plan.g_g;
            } else {
                hipLaunchKernelGGL(pose_grad_kernel, dim3(plan.g_g, b), dim3(kQBlock), 0, sn, nc, complete, (const float *)center,
                                   4, (const float *)Sc->params, kStateFloats, np, partial, (const float *)d1,
                                   (const int *)i1, (const float *)d2, (const int *)i2, 3.0f, ac, ho.ctr());
                ho.after_grad((unsigned)plan.g_g * (unsigned)b);
            }
            // 5. silhouette
            if (mask && !mask_step(b, nc, complete, complete_col, center, 4, Sc->params, kStateFloats, radius, render_size,
                                   mask_weight, m, ac, st, true, plan.ride ? &pga : nullptr))
                return 0;
            // 6. join, 7. update (fused: the next transform takes the update; the last step's is the launch below, in place)
            ho.join(it == iters);
            if (!plan.fuse_upd || it == iters)
                hipLaunchKernelGGL(pose_update_kernel, dim3(gb), dim3(64), 0, st, b, Sc, ac, nc, np, 3.0f, 0.001f, lr, 1, hslot, hstride);
        }
        // the start's final state back into the first set (where the kernels after the loop, and the next start, look for it)
        if (plan.fuse_upd && (iters & 1) && !check(hipMemcpyAsync(Sb[0], Sb[1], (size_t)b * sizeof(PoseState), hipMemcpyDeviceToDevice, st), "copy pose state")) return 0;
        // (the set the last transform read still holds the step before last's sums: the next start begins with both sets clear)
        if (plan.fuse_upd && iters > 0 && !check(hipMemsetAsync(ab[(iters & 1) ^ 1], 0, (size_t)b * kAcc * sizeof(double), st), "hipMemsetAsync(accumulators)")) return 0;
        hipLaunchKernelGGL(pose_end_kernel, dim3(gb), dim3(64), 0, st, b, S, 0, (float *)nullptr, (float *)nullptr);
    }
    if (plan.lock)
        hipLaunchKernelGGL(pose_pick_kernel, dim3(ceil_div(scans, 64)), dim3(64), 0, st, scans, starts_in, (const PoseState *)S, transform,
                           best_params);
    else
        hipLaunchKernelGGL(pose_end_kernel, dim3(gb), dim3(64), 0, st, b, S, 1, transform, best_params);
    ho.end();
    return check(hipGetLastError(), "pose_optimize launch") ? 1 : 0;
}

GENPC_API int genpc_pose_optimize_cd_batch(int b, int nc, const float *complete, int np, const float *partial,
                                           float lr, int iters, int starts, float *transform, float *history,
                                           float *best_params, void *stream)
{
    return genpc_pose_optimize_batch(b, nc, complete, nullptr, np, partial, nullptr, lr, iters, starts, 0.0f, 0, 0.0f,
                                     transform, history, best_params, stream);
}

GENPC_API int genpc_pose_optimize_cd(int nc, const float *complete, int np, const float *partial, float lr,
                                     int iters, int starts, float *transform, float *history, float *best_params,
                                     void *stream)
{
    return genpc_pose_optimize_cd_batch(1, nc, complete, np, partial, lr, iters, starts, transform, history,
                                        best_params, stream);
}

// One step of the loop for b elements, each with its own parameters, and no Adam step: the batched counterpart of
// genpc_pose_loss_grad, as genpc_pose_optimize_batch is of the single-scan loop.  The launches are the loop's at b elements on
// one stream (ask: scans = b, one start, no side stream, the switches at their defaults), every width from the two plans -- so
// the forms the plans select for wide calls (one lane per point, whole images per XCD, capped pose_grad grids, gb > 1) can be
// compared with an independent reference element by element (tests/test_gpu_pose_step_batch.py).
GENPC_API int genpc_pose_loss_grad_batch(int b, int nc, const float *v, const float *vert_col, const float *center, const float *params,
                                         int np, const float *partial, const float *partial_col, float cd_weight, float reg_weight,
                                         float mask_weight, float radius, int render_size, float *loss_out, float *grad, void *stream)
{
    using namespace genpc;
    if (b <= 0 || nc <= 0 || np <= 0) return -1;
    const bool mask = mask_weight != 0.0f;
    if (mask && (render_size <= 1 || !(radius > 0.0f))) return -1;
    hipStream_t st = (hipStream_t)stream;
    PoseLoopAsk ask;
    ask.scans = b; ask.starts = 1; ask.nc = nc; ask.np = np; ask.mask = mask;
    ask.side_stream_ok = false;
    ask.counters_ok = false;
    const PoseLoopPlan plan = pose_loop_plan(ask);

    const size_t P = mask ? (size_t)render_size * render_size : 0;
    double *accum; PoseState *S; float *pts, *d1, *d2; int *i1, *i2;
    MaskScratch m = {};
    WsLayout L;
    L.add(accum, (size_t)b * kAcc);
    L.add(S, (size_t)b);
    L.add(pts, (size_t)b * nc * 3);
    L.add(d1, (size_t)b * nc);
    L.add(d2, (size_t)b * np);
    L.add(i1, (size_t)b * nc);
    L.add(i2, (size_t)b * np);
    if (mask) m.layout(L, b, P, (size_t)(nc > np ? nc : np));
    if (!ws_alloc(L, kWsPoseLossGradBatch, st)) return 0;
    if (mask && !m.zero_bins(st)) return 0;
    constexpr int kStateFloats = (int)(sizeof(PoseState) / sizeof(float));
    if (!check(hipMemsetAsync(accum, 0, (size_t)b * kAcc * sizeof(double), st), "hipMemsetAsync(accum)")) return 0;
    if (!check(hipMemcpy2DAsync(S->params, sizeof(PoseState), params, 10 * sizeof(float), 10 * sizeof(float), (size_t)b, hipMemcpyDeviceToDevice, st),
               "copy params"))
        return 0;
    // reference image of the partial clouds: first, as in the loop (it projects through the scratch the transform then fills)
    if (mask && !mask_prepare_ref(b, np, partial, partial_col, radius, render_size, m, st)) return 0;
    // 1. transform (with the projection, for the full objective)
    if (mask) {
        PoseFuse fu{};
        hipLaunchKernelGGL(pose_transform_project_kernel, dim3(plan.g_t, b), dim3(kQBlock), 0, st, nc, v, center, 3, (const float *)S->params,
                           kStateFloats, pts, 1.1f * radius, render_size, m.uvr, use_bins(render_size) ? m.bins : (int *)nullptr,
                           render_blend() ? m.zex : (float *)nullptr, fu);
    } else
        hipLaunchKernelGGL(pose_transform_kernel, dim3(plan.g_t, b), dim3(kQBlock), 0, st, nc, v, center, 3, (const float *)S->params,
                           kStateFloats, pts);
    // 2. nearest neighbours, both directions.  (The loop makes the duplicate masks of both clouds once per call and hands them to every
    // step's search; one step is one search, so nn_forward is left to make its own where its policy wants them: the same bits.)
    if (nn_forward(b, 2, pts, nc, partial, np, d1, i1, partial, np, pts, nc, d2, i2, st) != 1) return 0;
    // 3. the Chamfer gradient: a launch of its own, or its blocks at the end of the silhouette gradient's launch
    PoseGradArgs pga{};
    if (plan.ride) {
        pga.nc = nc; pga.cstride = 3; pga.pstride = kStateFloats; pga.np = np;
        pga.v = v; pga.center = center; pga.params = S->params; pga.partial = partial;
        pga.d1 = d1; pga.d2 = d2; pga.i1 = i1; pga.i2 = i2;
        pga.cd_weight = cd_weight; pga.accum = accum; pga.gx = plan.g_g;
    } else
        hipLaunchKernelGGL(pose_grad_kernel, dim3(plan.g_g, b), dim3(kQBlock), 0, st, nc, v, center, 3, (const float *)S->params, kStateFloats,
                           np, partial, (const float *)d1, (const int *)i1, (const float *)d2, (const int *)i2, cd_weight, accum,
                           (unsigned *)nullptr);
    // 4. silhouette
    if (mask && !mask_step(b, nc, v, vert_col, center, 3, S->params, kStateFloats, radius, render_size, mask_weight, m, accum, st, true,
                           plan.ride ? &pga : nullptr))
        return 0;
    // 5. the gradient finished per element, no step taken
    hipLaunchKernelGGL(pose_update_kernel, dim3(plan.gb), dim3(64), 0, st, b, S, accum, nc, np, cd_weight, reg_weight, 0.0f, 0,
                       (float *)nullptr, 0);
    if (!check(hipMemcpy2DAsync(grad, 10 * sizeof(float), S->grad, sizeof(PoseState), 10 * sizeof(float), (size_t)b, hipMemcpyDeviceToDevice, st),
               "copy grad"))
        return 0;
    if (!check(hipMemcpy2DAsync(loss_out, 4 * sizeof(float), S->loss, sizeof(PoseState), 4 * sizeof(float), (size_t)b, hipMemcpyDeviceToDevice, st),
               "copy loss"))
        return 0;
    return check(hipGetLastError(), "pose_loss_grad_batch launch") ? 1 : 0;
}

// One step of the loop's seeded nearest-neighbour search on the caller's inputs, so that nn_seeded_kernel can be compared with a
// reference query by query (tests/test_gpu_nn_seeded.py): the loop's own three functions in the loop's order -- both grids
// (build_seeded_grids), the transform at the loop's width (pose_loop_plan's g_t), ONE launch_nn_seeded with i1 / i2 as seeds --
// in the calling thread's arithmetic mode.  Nothing of them is restated here and the kernel has no switch for it.
GENPC_API int genpc_nn_seeded_step(int b, int nm, const float *rest, const float *center, const float *params, int ns, const float *stat,
                                   float *posed, float *d1, int *i1, float *d2, int *i2, int sample, void *stream)
{
    using namespace genpc;
    if (b <= 0 || nm <= 0 || ns <= 0 || sample < 1) {
        set_error("genpc_nn_seeded_step: b, nm and ns must be positive and sample at least 1");
        return -1;
    }
    hipStream_t st = (hipStream_t)stream;
    PoseLoopAsk ask;
    ask.scans = b; ask.starts = 1; ask.nc = nm; ask.np = ns; ask.mask = false;
    ask.side_stream_ok = false;
    ask.counters_ok = false;
    const PoseLoopPlan plan = pose_loop_plan(ask);
    SeededGrids sg{};
    WsLayout GL;
    seeded_grids_layout(GL, sg, b, nm, ns);
    if (!ws_alloc(GL, kWsNnSeededStep, st) || !build_seeded_grids(b, nm, rest, ns, stat, sg, st)) return 0;
    const int fma_mode = arith_mode() != 0 ? 1 : 0;
    hipLaunchKernelGGL(pose_transform_kernel, dim3(plan.g_t, b), dim3(kQBlock), 0, st, nm, rest, center, 3, params, 10, posed);
    if (launch_nn_seeded(b, nm, posed, ns, stat, sg, center, 3, params, 10, d1, i1, d2, i2, fma_mode, st, sample) != 1) return 0;
    return check(hipGetLastError(), "nn_seeded_step launch") ? 1 : 0;
}

// ---- the ragged loop: S scans of different sizes in one call (pose_ragged_plan.h; the kernels are the ones above, given a table) ----
namespace genpc {

// What a ragged pose call is refused for before it is planned (ragged_offsets.h's check; no empty cloud: a scan without points on
// either side has no objective).  1: go on; 0: no scan, nothing to do; -1: refused, the error recorded under fn's name.
static int pose_ragged_admit(const char *fn, int c, const int *coff, const int *poff, int starts, int iters, bool mask, int render_size,
                             float radius)
{
    if (c < 0) return ragged_refuse(fn, "negative number of scans");
    if (c == 0) return 0;
    if (!coff || !poff) return ragged_refuse(fn, "null offset table");
    if (starts < 1 || iters < 0) return ragged_refuse(fn, "starts must be at least 1 and iters at least 0");
    if (mask && (render_size <= 1 || !(radius > 0.0f))) return ragged_refuse(fn, "the full objective needs render_size > 1 and a positive radius");
    if (const char *err = ragged_offsets_fault(c, {coff, poff})) return ragged_refuse(fn, err);
    for (int j = 0; j < c; j++) {
        const bool no_c = coff[j + 1] == coff[j], no_p = poff[j + 1] == poff[j];
        if (no_c || no_p) {
            char msg[96];
            snprintf(msg, sizeof msg, "scan %d has an empty %s cloud", j, no_c ? "complete" : "partial");
            return ragged_refuse(fn, msg);
        }
    }
    return 1;
}

// The tables of a planned call, by value: the scans' (replication), and the elements' in the two directions of the search --
// posed -> partial (queries by coff_e, targets by poff_e) and partial -> posed.
struct PoseRaggedTables {
    RaggedTable scans, fwd, bwd;
};
static void pose_ragged_fill(int c, const int *coff, const int *poff, int starts, PoseRaggedTables &T)
{
    int ce[kRaggedMaxPairs + 1], pe[kRaggedMaxPairs + 1];
    const int elements = c * starts;
    pose_ragged_element_offsets(c, coff, starts, ce);
    pose_ragged_element_offsets(c, poff, starts, pe);
    T.scans.c = c;
    ragged_pad_copy(T.scans.qoff, coff, c);
    ragged_pad_copy(T.scans.toff, poff, c);
    T.fwd.c = T.bwd.c = elements;
    ragged_pad_copy(T.fwd.qoff, ce, elements);
    ragged_pad_copy(T.fwd.toff, pe, elements);
    ragged_pad_copy(T.bwd.qoff, pe, elements);
    ragged_pad_copy(T.bwd.toff, ce, elements);
}

// The pieces both entry points lay out alike, behind their accumulators and states
struct PoseRaggedScratch {
    int *coff_e, *poff_e;          // the element tables on the device
    float *pts, *d1, *d2;
    int *i1, *i2;
    void layout(WsLayout &L, int elements, size_t total_c, size_t total_p)
    {
        L.add(coff_e, (size_t)elements + 1);
        L.add(poff_e, (size_t)elements + 1);
        L.add(pts, total_c * 3);
        L.add(d1, total_c);
        L.add(d2, total_p);
        L.add(i1, total_c);
        L.add(i2, total_p);
    }
};

// One step's launches between the transform and the update, the same in the loop and in the single step: nearest neighbours in both
// directions from the grid search (the partial clouds' grids are built by the caller, once; the posed clouds' here, every step),
// the Chamfer gradient (riding or alone), the silhouette step.
static int pose_ragged_step(const PoseRaggedPlan &plan, const PoseRaggedTables &T, const PoseRaggedScratch &x, const NnRaggedGrids &grid_partial,
                            const NnRaggedGrids &grid_posed, const float *complete, const float *complete_col, const float *partial,
                            const float *center, int cstride, const float *params, int pstride, float cd_weight, float mask_weight, float radius,
                            int render_size, const MaskScratch &m, double *accum, hipStream_t st)
{
    const int b = plan.elements;
    if (plan.nn_dense) {              // all pairs: two launches on the clouds as they lie, no grid (the same bits)
        if (nn_ragged_dense(T.fwd, x.pts, partial, x.d1, x.i1, st) != 1) return 0;
        if (nn_ragged_dense(T.bwd, partial, x.pts, x.d2, x.i2, st) != 1) return 0;
    } else {
        if (nn_ragged_search(T.fwd, x.pts, grid_partial, x.d1, x.i1, st) != 1) return 0;
        if (nn_ragged_build(T.bwd, plan.nc_max, x.pts, grid_posed, st) != 1) return 0;
        if (nn_ragged_search(T.bwd, partial, grid_posed, x.d2, x.i2, st) != 1) return 0;
    }
    PoseGradArgs pga{};
    if (plan.ride) {
        pga.nc = plan.nc_max; pga.cstride = cstride; pga.pstride = pstride; pga.np = plan.np_max;
        pga.v = complete; pga.center = center; pga.params = params; pga.partial = partial;
        pga.d1 = x.d1; pga.d2 = x.d2; pga.i1 = x.i1; pga.i2 = x.i2;
        pga.cd_weight = cd_weight; pga.accum = accum; pga.gx = plan.g_g;
        pga.coff = x.coff_e; pga.poff = x.poff_e;
    } else {
        hipLaunchKernelGGL(pose_grad_kernel, dim3(plan.g_g, b), dim3(kQBlock), 0, st, plan.nc_max, complete, center, cstride, params, pstride,
                           plan.np_max, partial, (const float *)x.d1, (const int *)x.i1, (const float *)x.d2, (const int *)x.i2, cd_weight, accum,
                           (unsigned *)nullptr, (const int *)x.coff_e, (const int *)x.poff_e);
    }
    if (mask_weight != 0.0f && !mask_step(b, plan.nc_max, complete, complete_col, center, cstride, params, pstride, radius, render_size, mask_weight, m,
                                          accum, st, true, plan.ride ? &pga : nullptr, x.coff_e, &plan.step))
        return 0;
    return 1;
}

// the transform of a step (with the projection, for the full objective)
static void pose_ragged_transform(const PoseRaggedPlan &plan, const PoseRaggedScratch &x, const float *complete, const float *center, int cstride,
                                  const float *params, int pstride, bool mask, float radius, int render_size, const MaskScratch &m, hipStream_t st)
{
    if (mask) {
        PoseFuse fu{};
        hipLaunchKernelGGL(pose_transform_project_kernel, dim3(plan.g_t, plan.elements), dim3(kQBlock), 0, st, plan.nc_max, complete, center, cstride,
                           params, pstride, x.pts, 1.1f * radius, render_size, m.uvr, use_bins(render_size) ? m.bins : (int *)nullptr,
                           render_blend() ? m.zex : (float *)nullptr, fu, (const int *)x.coff_e);
    } else
        hipLaunchKernelGGL(pose_transform_kernel, dim3(plan.g_t, plan.elements), dim3(kQBlock), 0, st, plan.nc_max, complete, center, cstride, params,
                           pstride, x.pts, (const int *)x.coff_e);
}

// both directions' grids, each in the slot of its direction
static bool pose_ragged_grids(const PoseRaggedTables &T, NnRaggedGrids &grid_partial, NnRaggedGrids &grid_posed, hipStream_t st)
{
    WsLayout LP, LC;
    nn_ragged_grids_layout(LP, grid_partial, T.fwd);
    nn_ragged_grids_layout(LC, grid_posed, T.bwd);
    return ws_alloc(LP, kWsPoseRaggedGridPartial, st) && ws_alloc(LC, kWsPoseRaggedGridPosed, st);
}

// What the all-pairs search refuses of a planned call (nn_ragged_dense_plan.h: both directions count the same pair evaluations,
// and each side is the other's targets), by the entry point's name; null when it takes the call.
static const char *pose_ragged_dense_refusal(const PoseRaggedTables &T)
{
    if (const char *why = nn_ragged_dense_plan(T.fwd).too_large) return why;
    return nn_ragged_dense_plan(T.bwd).too_large;
}

}  // namespace genpc

GENPC_API int genpc_pose_ragged_plan(int c, const int *coff, const int *poff, int starts, int mask, int render_size, float radius, int cus,
                                     int out[16])
{
    using namespace genpc;
    const char *fn = "genpc_pose_ragged_plan";
    if (!out) return ragged_refuse(fn, "null output");
    for (int k = 0; k < 16; k++) out[k] = 0;
    const int rc = pose_ragged_admit(fn, c, coff, poff, starts, 0, mask != 0, render_size, radius);
    if (rc <= 0) return rc < 0 ? -1 : 1;
    PoseRaggedAsk ask;
    ask.c = c; ask.coff = coff; ask.poff = poff; ask.starts = starts; ask.mask = mask != 0; ask.render_size = render_size; ask.radius = radius;
    ask.cus = cus;
    const PoseRaggedPlan plan = pose_ragged_plan(ask);
    const long long cap = 0x7fffffffll;
    out[0] = plan.elements; out[1] = plan.nc_max; out[2] = plan.np_max; out[3] = plan.g_t; out[4] = plan.g_g; out[5] = plan.gb;
    out[6] = plan.g_m; out[7] = plan.ride; out[8] = plan.step.fuse_w; out[9] = plan.step.sub8; out[10] = plan.step.gp; out[11] = plan.step.gs;
    out[12] = plan.too_large ? 1 : 0;
    out[13] = (int)std::min(plan.total_c, cap); out[14] = (int)std::min(plan.total_p, cap);
    out[15] = plan.blocks_per_cu;
    return 1;
}

GENPC_API int genpc_pose_loss_grad_ragged(int c, const int *coff, const int *poff, const float *v, const float *vert_col, const float *center,
                                          const float *params, const float *partial, const float *partial_col, float cd_weight, float reg_weight,
                                          float mask_weight, float radius, int render_size, float *loss_out, float *grad, void *stream)
{
    using namespace genpc;
    const char *fn = "genpc_pose_loss_grad_ragged";
    const bool mask = mask_weight != 0.0f;
    const int rc = pose_ragged_admit(fn, c, coff, poff, 1, 0, mask, render_size, radius);
    if (rc <= 0) return rc < 0 ? -1 : 1;
    hipStream_t st = (hipStream_t)stream;
    PoseRaggedAsk ask;
    ask.c = c; ask.coff = coff; ask.poff = poff; ask.starts = 1; ask.mask = mask; ask.render_size = render_size; ask.radius = radius;
    ask.cus = num_cus();
    ask.nn_dense = t_nn_ragged_dense;
    const PoseRaggedPlan plan = pose_ragged_plan(ask);
    if (plan.too_large) return ragged_refuse(fn, plan.too_large);
    if (!v || !center || !params || !partial || !loss_out || !grad) return ragged_refuse(fn, "null pointer");
    PoseRaggedTables T;
    pose_ragged_fill(c, coff, poff, 1, T);
    if (plan.nn_dense)
        if (const char *why = pose_ragged_dense_refusal(T)) return ragged_refuse(fn, why);
    const int b = plan.elements;

    const size_t P = mask ? (size_t)render_size * render_size : 0;
    double *accum; PoseState *S;
    PoseRaggedScratch x{};
    MaskScratch m = {};
    WsLayout L;
    L.add(accum, (size_t)b * kAcc);
    L.add(S, (size_t)b);
    x.layout(L, b, (size_t)plan.total_c, (size_t)plan.total_p);
    if (mask) m.layout(L, b, P, (size_t)plan.nmax_piece);
    if (!ws_alloc(L, kWsPoseRaggedStep, st)) return 0;
    NnRaggedGrids grid_partial{}, grid_posed{};
    if (!plan.nn_dense && !pose_ragged_grids(T, grid_partial, grid_posed, st)) return 0;          // (all pairs: neither slot is taken)
    if (mask && !m.zero_bins(st)) return 0;
    constexpr int kStateFloats = (int)(sizeof(PoseState) / sizeof(float));
    if (!check(hipMemsetAsync(accum, 0, (size_t)b * kAcc * sizeof(double), st), "hipMemsetAsync(accum)")) return 0;
    if (!check(hipMemcpy2DAsync(S->params, sizeof(PoseState), params, 10 * sizeof(float), 10 * sizeof(float), (size_t)b, hipMemcpyDeviceToDevice, st),
               "copy params"))
        return 0;
    if (!pose_ragged_tables(T.fwd, x.coff_e, x.poff_e, st)) return 0;
    // the order of genpc_pose_loss_grad_batch: reference images first (they project through the scratch the transform then fills)
    if (mask && !mask_prepare_ref(b, plan.np_max, partial, partial_col, radius, render_size, m, st, x.poff_e)) return 0;
    if (!plan.nn_dense && nn_ragged_build(T.fwd, plan.np_max, partial, grid_partial, st) != 1) return 0;
    pose_ragged_transform(plan, x, v, center, 3, S->params, kStateFloats, mask, radius, render_size, m, st);
    if (!pose_ragged_step(plan, T, x, grid_partial, grid_posed, v, vert_col, partial, center, 3, S->params, kStateFloats, cd_weight, mask_weight, radius,
                          render_size, m, accum, st))
        return 0;
    hipLaunchKernelGGL(pose_update_kernel, dim3(plan.gb), dim3(64), 0, st, b, S, accum, plan.nc_max, plan.np_max, cd_weight, reg_weight, 0.0f, 0,
                       (float *)nullptr, 0, (const int *)x.coff_e, (const int *)x.poff_e);
    if (!check(hipMemcpy2DAsync(grad, 10 * sizeof(float), S->grad, sizeof(PoseState), 10 * sizeof(float), (size_t)b, hipMemcpyDeviceToDevice, st),
               "copy grad"))
        return 0;
    if (!check(hipMemcpy2DAsync(loss_out, 4 * sizeof(float), S->loss, sizeof(PoseState), 4 * sizeof(float), (size_t)b, hipMemcpyDeviceToDevice, st),
               "copy loss"))
        return 0;
    return check(hipGetLastError(), "pose_loss_grad_ragged launch") ? 1 : 0;
}

GENPC_API int genpc_pose_optimize_ragged(int c, const int *coff, const int *poff, const float *complete, const float *complete_col,
                                         const float *partial, const float *partial_col, float lr, int iters, int starts, float radius,
                                         int render_size, float mask_weight, float *transform, float *history, float *best_params, void *stream)
{
    using namespace genpc;
    const char *fn = "genpc_pose_optimize_ragged";
    const bool mask = mask_weight != 0.0f;
    const int rc = pose_ragged_admit(fn, c, coff, poff, starts, iters, mask, render_size, radius);
    if (rc <= 0) return rc < 0 ? -1 : 1;
    hipStream_t st = (hipStream_t)stream;
    PoseRaggedAsk ask;
    ask.c = c; ask.coff = coff; ask.poff = poff; ask.starts = starts; ask.mask = mask; ask.render_size = render_size; ask.radius = radius;
    ask.cus = num_cus();
    ask.nn_dense = t_nn_ragged_dense;
    const PoseRaggedPlan plan = pose_ragged_plan(ask);
    if (plan.too_large) return ragged_refuse(fn, plan.too_large);
    if (!complete || !partial || !transform) return ragged_refuse(fn, "null pointer");
    PoseRaggedTables T;
    pose_ragged_fill(c, coff, poff, starts, T);
    if (plan.nn_dense)
        if (const char *why = pose_ragged_dense_refusal(T)) return ragged_refuse(fn, why);
    const int b = plan.elements;

    // every cloud once per start, packed by the element tables (as pose_replicate does for equal sizes); the pointers move there
    if (plan.replicate) {
        float *xs[4];
        const size_t xc = (size_t)plan.total_c * 3, xp = (size_t)plan.total_p * 3;
        WsLayout X;          // (the colours' pieces are reserved whether or not the call brings colours)
        X.add(xs[0], xc);
        X.add(xs[1], xp);
        X.add(xs[2], xc);
        X.add(xs[3], xp);
        if (!ws_alloc(X, kWsPoseRaggedReplicas, st)) return 0;
        const float *src[4] = {complete, partial, complete_col, partial_col};
        if (!pose_ragged_replicate(T.scans, starts, plan.g_rep, src, xs, st)) return 0;
        complete = xs[0]; partial = xs[1];
        complete_col = complete_col ? xs[2] : nullptr; partial_col = partial_col ? xs[3] : nullptr;
    }

    const size_t P = mask ? (size_t)render_size * render_size : 0;
    double *accum; PoseState *S; float *center;
    PoseRaggedScratch x{};
    MaskScratch m = {};
    WsLayout L;
    L.add(accum, (size_t)b * kAcc);
    L.add(S, (size_t)b);
    L.add(center, (size_t)b * 4);
    x.layout(L, b, (size_t)plan.total_c, (size_t)plan.total_p);
    if (mask) m.layout(L, b, P, (size_t)plan.nmax_piece);
    if (!ws_alloc(L, kWsPoseRaggedLoop, st)) return 0;
    NnRaggedGrids grid_partial{}, grid_posed{};
    if (!plan.nn_dense && !pose_ragged_grids(T, grid_partial, grid_posed, st)) return 0;          // (all pairs: neither slot is taken)
    if (mask && !m.zero_bins(st)) return 0;
    constexpr int kStateFloats = (int)(sizeof(PoseState) / sizeof(float));
    if (!pose_ragged_tables(T.fwd, x.coff_e, x.poff_e, st)) return 0;

    // center = mean(vert_pos) per element (diff_obj_pose.py:362); the reference images; the partial clouds' grids: once per call
    if (!genpc_mean3(b, plan.nc_max, complete, center, accum, st, x.coff_e)) return 0;
    if (mask && !mask_prepare_ref(b, plan.np_max, partial, partial_col, radius, render_size, m, st, x.poff_e)) return 0;
    if (!plan.nn_dense && nn_ragged_build(T.fwd, plan.np_max, partial, grid_partial, st) != 1) return 0;

    hipLaunchKernelGGL(pose_begin_kernel, dim3(plan.gb), dim3(64), 0, st, b, S, accum, -1, 0);
    hipLaunchKernelGGL(pose_begin_kernel, dim3(plan.gb), dim3(64), 0, st, b, S, accum, 0, starts);
    const int hstride = iters + 1;          // history [c, starts, iters + 1]: element e's row is e
    for (int it = 0; it <= iters; it++) {
        pose_ragged_transform(plan, x, complete, center, 4, S->params, kStateFloats, mask, radius, render_size, m, st);
        if (!pose_ragged_step(plan, T, x, grid_partial, grid_posed, complete, complete_col, partial, center, 4, S->params, kStateFloats, 3.0f,
                              mask_weight, radius, render_size, m, accum, st))
            return 0;
        hipLaunchKernelGGL(pose_update_kernel, dim3(plan.gb), dim3(64), 0, st, b, S, accum, plan.nc_max, plan.np_max, 3.0f, 0.001f, lr, 1,
                           history ? history + it : (float *)nullptr, hstride, (const int *)x.coff_e, (const int *)x.poff_e);
    }
    // the start picked per scan: pose_pick_kernel's rule, the equal-size loop's
    hipLaunchKernelGGL(pose_pick_kernel, dim3(ceil_div(c, 64)), dim3(64), 0, st, c, starts, (const PoseState *)S, transform, best_params);
    return check(hipGetLastError(), "pose_optimize_ragged launch") ? 1 : 0;
}

namespace genpc {

// accum[e*kAcc + 0..2] += sum of v[e, :, 0..2]
__global__ __launch_bounds__(kQBlock) void mean3_accum_kernel(int n, const float *__restrict__ v,
                                                              double *__restrict__ accum, const int *__restrict__ off = nullptr)
{
    __shared__ double red[3][kQBlock / kWave];
    const int e = blockIdx.y;
    const PoseSpan sp = pose_span(off, e, n);
    n = sp.n;
    if (off && (int)blockIdx.x * kQBlock >= n) return;       // a short element of a ragged call: the whole block leaves
    v += sp.base * 3;
    accum += (size_t)e * kAcc;
    double a[3] = {0.0, 0.0, 0.0};
    for (int j = blockIdx.x * kQBlock + threadIdx.x; j < n; j += gridDim.x * kQBlock) {
        a[0] += (double)v[(size_t)j * 3 + 0];
        a[1] += (double)v[(size_t)j * 3 + 1];
        a[2] += (double)v[(size_t)j * 3 + 2];
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double x = wave_sum63(a[k]);
        if (lane == kWave - 1) red[k][wave] = x;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double x = 0.0;
        for (int w2 = 0; w2 < kQBlock / kWave; w2++) x += red[threadIdx.x][w2];
        atomicAdd(&accum[threadIdx.x], x);
    }
}

__global__ void mean3_finish_kernel(int b, int n, double *__restrict__ accum, float *__restrict__ out,
                                    const int *__restrict__ off = nullptr)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= b * 3) return;
    const int e = t / 3, k = t % 3;
    n = pose_span(off, e, n).n;
    out[e * 4 + k] = (float)(accum[(size_t)e * kAcc + k] / n);
    accum[(size_t)e * kAcc + k] = 0.0;
}

// (off: a ragged call's element table on the device, n then the largest element's count -- the launch's width)
int genpc_mean3(int b, int n, const float *v, float *out, double *accum, hipStream_t st, const int *off)
{
    if (!check(hipMemsetAsync(accum, 0, (size_t)b * kAcc * sizeof(double), st), "hipMemsetAsync(mean)")) return 0;
    hipLaunchKernelGGL(mean3_accum_kernel, dim3(lin_grid(n), b), dim3(kQBlock), 0, st, n, v, accum, off);
    hipLaunchKernelGGL(mean3_finish_kernel, dim3(ceil_div(b * 3, 64)), dim3(64), 0, st, b, n, accum, out, off);
    return check(hipGetLastError(), "mean3 launch") ? 1 : 0;
}

}  // namespace genpc
