// fps_verify.hip -- the check every farthest-point sampling of the library gets, whichever of the three samplers drew it
// (fps_grid.hip, fps.hip, fps_large.hip): the chip-wide verification kernel, its in-line form (fps_verify) and the deferred
// form on a side stream (fps_verify_deferred, genpc_fps_defer, genpc_fps_deferred_check).  How many segments a check is cut
// into and the layout of a deferred check's buffer are fps_plan.h's.
#include "fps.h"
#include "../../include/genpc_hip.h"
#include <map>
#include <mutex>

namespace genpc {

// Verification of a sampling, on the device, against the DEFINITION (round 5).  The k steps of a sampling are sequential, but
// checking a finished sequence is not: sample j (drawn with running minimum M_j, as the sampling itself recorded it) is right
// iff, after the first j samples have been applied, every point i has running minimum D_i < M_j, or D_i == M_j and i > s_j,
// and the sample itself has D == M_j exactly -- "s_j is the FIRST arg-max" -- with the sampling's own arithmetic.  One thread
// per point walks the sample list once (n k distance evaluations, all independent across points: ~0.4 ms for 16384 of 24000,
// beside the sampling's 7).  Why: twice now (round 4 next to another stream's f16 MFMAs, round 5 again with the pivot taken
// through scalar registers and with self-tagged pivot granules) a sampling running BESIDE other kernels drew a sample a step
// early -- silently, mechanism not established.  A violation poisons out[0] with -1, which genpc_amd/fps.py
// already treats as "this cloud again": a wrong sequence can no longer leave the library unnoticed, whatever causes it.
constexpr int kFVTile = 1024;          // samples staged in LDS at a time (kFVBlock, kFVMaxSeg: fps_plan.h)
// The sample list is cut into `nseg` segments (grid.z) so that the whole chip takes part (one thread per point alone
// leaves a 24000-point cloud on 188 two-wave blocks: 1.8 ms beside a 10 ms sampling).  CHECK = 0: the minimum over the
// segment's samples of the point's distances -> segmin[point][segment]; CHECK = 1: the running minimum enters the segment
// with the minimum of the earlier segments' results and the segment's steps are checked.  Twice the distance
// evaluations, nseg times the threads.
template <int FMA, int CHECK>
__global__ __launch_bounds__(kFVBlock) void fps_verify_kernel(FpsJobs jobs, float *__restrict__ segmin, int nseg)
{
    __shared__ float4 s_s[kFVTile];          // x, y, z of sample l; M of sample l + 1
    __shared__ int s_i[kFVTile];             // index of sample l + 1
    __shared__ unsigned s_hit[kFVTile / 256];      // per trip of eight samples: one of them is a point of this block
    const int job = blockIdx.y, seg = blockIdx.z;
    const int n = jobs.n[job], k = jobs.k[job];
    const float *__restrict__ X = jobs.xyz[job];
    const int *__restrict__ out = jobs.out[job];
    const float *__restrict__ pd = jobs.pdist[job];
    float *__restrict__ sm = segmin + (size_t)jobs.segoff[job] * nseg;
    // samples l = 0 .. k - 2 are applied (sample l decides step l + 1); the segment's share, a multiple of 8 long
    const int per = (((k - 1) + nseg - 1) / nseg + 7) & ~7;
    const int l_lo = min(seg * per, k - 1), l_hi = min(l_lo + per, k - 1);
    bool bad = false;
    for (int i0 = blockIdx.x * kFVBlock; i0 < n; i0 += gridDim.x * kFVBlock) {      // (block-uniform: the tiles are staged together)
        const int i = min(i0 + (int)threadIdx.x, n - 1);      // (lanes past the end repeat the last point)
        const float px = X[(size_t)i * 3 + 0], py = X[(size_t)i * 3 + 1], pz = X[(size_t)i * 3 + 2];
        float D = __builtin_inff();
        if (CHECK) {
            for (int g = 0; g < seg; g++) D = fminf(D, sm[(size_t)i * nseg + g]);
            if (i == 0 && seg == 0 && out[0] != 0) bad = true;      // (-1: the hand-off gave up; anything else: not the start point)
        }
        for (int l0 = l_lo; l0 < l_hi; l0 += kFVTile) {
            __syncthreads();
            if (CHECK && threadIdx.x < kFVTile / 256) s_hit[threadIdx.x] = 0u;
            if (CHECK) __syncthreads();
            for (int t = threadIdx.x; t < kFVTile && l0 + t < l_hi; t += kFVBlock) {
                int sl = out[l0 + t];
                if (CHECK && ((unsigned)sl >= (unsigned)n || (unsigned)out[l0 + t + 1] >= (unsigned)n)) bad = true;      // (not an index of the cloud)
                sl = (unsigned)sl < (unsigned)n ? sl : 0;
                s_s[t] = make_float4(X[(size_t)sl * 3 + 0], X[(size_t)sl * 3 + 1], X[(size_t)sl * 3 + 2], pd[l0 + t + 1]);
                const int sn = out[l0 + t + 1];
                s_i[t] = sn;
                if (CHECK && (unsigned)(sn - i0) < (unsigned)kFVBlock) atomicOr(&s_hit[t >> 8], 1u << ((t >> 3) & 31));
            }
            __syncthreads();
            const int cnt = min(kFVTile, l_hi - l0);
            // eight samples per trip: the LDS reads (broadcasts) and the eight independent distances first, then the
            // running minimum's short dependent chain
            int t = 0;
            for (; t + 8 <= cnt; t += 8) {
                float4 q[8];
                float dd[8];
#pragma unroll
                for (int u = 0; u < 8; u++) q[u] = s_s[t + u];
#pragma unroll
                for (int u = 0; u < 8; u++) dd[u] = sqdist<FMA>(px - q[u].x, py - q[u].y, pz - q[u].z);
                if (!CHECK) {
#pragma unroll
                    for (int u = 0; u < 8; u++) D = D < dd[u] ? D : dd[u];
                    continue;
                }
                // the common case costs one comparison per step: D < M.  A step with D >= M -- the sample itself (D == M), an exact
                // tie, or a violation -- is rare and looked at again below with the index rule
                const float D0 = D;
                bool ge = false;
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    D = D < dd[u] ? D : dd[u];
                    ge |= D >= q[u].w;
                }
                // (a sample whose recorded minimum is too HIGH has D < M at its own step: the trips in which a point of THIS block
                // is sampled are marked while the tile is staged and take the full rule whatever the comparison says)
                const bool hit = CHECK && ((s_hit[t >> 8] >> ((t >> 3) & 31)) & 1u) != 0u;
                if (hit || __any(ge)) {
                    float E = D0;
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        E = E < dd[u] ? E : dd[u];
                        const int sj = s_i[t + u];
                        // E < M, or the tie goes to the lower index s_j; and s_j itself has exactly its recorded minimum
                        bad |= !(E < q[u].w || (E == q[u].w && i >= sj)) || (i == sj && E != q[u].w);
                    }
                }
            }
            for (; t < cnt; t++) {
                const float4 q = s_s[t];
                const float dd = sqdist<FMA>(px - q.x, py - q.y, pz - q.z);
                D = D < dd ? D : dd;
                const int sj = s_i[t];
                if (CHECK) bad |= !(D < q.w || (D == q.w && i >= sj)) || (i == sj && D != q.w);
            }
        }
        if (!CHECK && i0 + (int)threadIdx.x < n) sm[(size_t)i * nseg + seg] = D;
    }
    if (CHECK && __any(bad) && (threadIdx.x & (kWave - 1)) == 0) atomicOr(jobs.verr[job], 1);      // (padding lanes repeat point n - 1: same verdict)
}

__global__ void fps_poison_kernel(FpsJobs jobs, int nj)
{
    const int j = threadIdx.x;
    // (-2: the sequence failed the check; a sampling whose hand-off timed out has written -1 itself, and fails the check too)
    if (j < nj && *jobs.verr[j] != 0) { if (jobs.out[j][0] != -1) jobs.out[j][0] = -2; *jobs.verr[j] = 0; }
}

// deferred verification (below): a failed check is counted instead of poisoning a result that has left already
__global__ void fps_count_kernel(FpsJobs jobs, int nj, int *__restrict__ violations)
{
    const int j = threadIdx.x;
    if (j < nj && *jobs.verr[j] != 0) { atomicAdd(violations, 1); *jobs.verr[j] = 0; }
}

// the check of a group of clouds on `st`; violations: the deferred form's counter, null in line (a failed check poisons out[0]);
// force_nseg: 0, or the number of segments to cut into whatever fps_verify_segments says (genpc_fps_verify_probe)
static void launch_verify(const FpsJobs &jobs, int nj, bool single, bool fma, int cus, hipStream_t st, float *segmin, int *violations,
                          int force_nseg)
{
    int nmax = 1;
    for (int q = 0; q < nj; q++) nmax = jobs.n[q] > nmax ? jobs.n[q] : nmax;
    const int nseg = force_nseg > 0 ? force_nseg : fps_verify_segments(nmax, nj, cus, single);
    const dim3 vg(ceil_div(nmax, kFVBlock), nj, nseg);
    if (nseg > 1) {
        if (fma) hipLaunchKernelGGL((fps_verify_kernel<1, 0>), vg, dim3(kFVBlock), 0, st, jobs, segmin, nseg);
        else hipLaunchKernelGGL((fps_verify_kernel<0, 0>), vg, dim3(kFVBlock), 0, st, jobs, segmin, nseg);
    }
    if (fma) hipLaunchKernelGGL((fps_verify_kernel<1, 1>), vg, dim3(kFVBlock), 0, st, jobs, segmin, nseg);
    else hipLaunchKernelGGL((fps_verify_kernel<0, 1>), vg, dim3(kFVBlock), 0, st, jobs, segmin, nseg);
    if (violations) hipLaunchKernelGGL(fps_count_kernel, dim3(1), dim3(kFMaxJobs), 0, st, jobs, nj, violations);
    else hipLaunchKernelGGL(fps_poison_kernel, dim3(1), dim3(kFMaxJobs), 0, st, jobs, nj);
}

void fps_verify(const FpsCall &c, const FpsJobs &jobs, int nj, bool single)
{
    launch_verify(jobs, nj, single, c.fma, c.cus, c.st, c.segmin, nullptr, 0);
}

// Verification OFF the caller's critical path (round 6; genpc_fps_defer).  The check of a finished sequence reads the cloud, the
// samples and their recorded minima: ~1 ms of chip-wide kernels behind a 4-5 ms sampling, twice per completed scan.  Deferred,
// the three arrays are copied (stream-ordered, ~0.5 MB) into a buffer of the library's own and the check runs on a side stream
// of the lowest priority class beside whatever the caller enqueues next; a failed check is COUNTED (the indices have left by
// then) and genpc_fps_deferred_check() hands the count to the caller, who samples again with the check in line
// (genpc_amd/pipeline.py does, per completed scan).  Only samplings of the one-workgroup kernel (csrc/fps_grid.hip) are
// deferred: the failures that made the check necessary were hand-offs between workgroups, which it does not have.
thread_local int t_fps_defer = 0;
struct FpsDeferred {
    hipStream_t side = nullptr;
    hipEvent_t fork[4] = {nullptr, nullptr, nullptr, nullptr}, done[4] = {nullptr, nullptr, nullptr, nullptr};
    char *buf[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t cap[4] = {0, 0, 0, 0};
    bool used[4] = {false, false, false, false};
    int *violations = nullptr;      // device word
    unsigned next = 0;
    bool ok = false;
};
static std::mutex g_fps_def_mu;
static std::map<std::pair<int, hipStream_t>, FpsDeferred *> g_fps_def;
FpsDeferred *fps_deferred_of(hipStream_t st, bool create)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> g(g_fps_def_mu);
    auto it = g_fps_def.find({dev, st});
    if (it != g_fps_def.end()) return it->second->ok ? it->second : nullptr;
    if (!create) return nullptr;
    FpsDeferred *p = new FpsDeferred();
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    p->ok = hipStreamCreateWithPriority(&p->side, hipStreamNonBlocking, prio_lo) == hipSuccess;
    for (int i = 0; i < 4 && p->ok; i++)
        p->ok = hipEventCreateWithFlags(&p->fork[i], hipEventDisableTiming) == hipSuccess &&
                hipEventCreateWithFlags(&p->done[i], hipEventDisableTiming) == hipSuccess;
    p->ok = p->ok && hipMalloc((void **)&p->violations, sizeof(int)) == hipSuccess && hipMemset(p->violations, 0, sizeof(int)) == hipSuccess;
    g_fps_def[{dev, st}] = p;
    return p->ok ? p : nullptr;
}

// deferred form: the group's arrays copied behind the sampling, the check on the side stream
bool fps_verify_deferred(const FpsCall &c, const FpsJobs &jobs, int nj, FpsDeferred *d)
{
    // (buffers of the check's own, not the pool's)
    const FpsDeferredLayout lay = fps_deferred_layout(nj, jobs.n, jobs.k);
    const size_t bytes = lay.bytes;
    hipStream_t st = c.st;
    const int sl = (int)(d->next++ & 3u);
    if (d->used[sl] && hipStreamWaitEvent(st, d->done[sl], 0) != hipSuccess) return false;       // (the slot's previous check: long finished)
    if (d->cap[sl] == 0 && !d->used[0] && !d->used[1] && !d->used[2] && !d->used[3]) {
        // first use: all four buffers at once (an allocation synchronises the device: not inside the caller's second and third call)
        for (int q = 0; q < 4; q++) {
            if (hipMalloc((void **)&d->buf[q], bytes + bytes / 4) != hipSuccess) return false;
            d->cap[q] = bytes + bytes / 4;
        }
    }
    if (d->cap[sl] < bytes) {
        if (d->buf[sl]) {
            if (hipStreamSynchronize(d->side) != hipSuccess || hipFree(d->buf[sl]) != hipSuccess) return false;
            d->buf[sl] = nullptr;
            d->cap[sl] = 0;
        }
        if (hipMalloc((void **)&d->buf[sl], bytes + bytes / 4) != hipSuccess) return false;
        d->cap[sl] = bytes + bytes / 4;
    }
    char *b = d->buf[sl];
    FpsJobs cp = jobs;
    if (hipMemsetAsync(b, 0, kFpsWsAlign, st) != hipSuccess) return false;
    for (int q = 0; q < nj; q++) {
        const size_t xb = (size_t)jobs.n[q] * 12, kb = (size_t)jobs.k[q] * 4;
        if (hipMemcpyAsync(b + lay.xyz[q], jobs.xyz[q], xb, hipMemcpyDeviceToDevice, st) != hipSuccess) return false;
        cp.xyz[q] = (const float *)(b + lay.xyz[q]);
        if (hipMemcpyAsync(b + lay.out[q], jobs.out[q], kb, hipMemcpyDeviceToDevice, st) != hipSuccess) return false;
        cp.out[q] = (int *)(b + lay.out[q]);
        if (hipMemcpyAsync(b + lay.pdist[q], jobs.pdist[q], kb, hipMemcpyDeviceToDevice, st) != hipSuccess) return false;
        cp.pdist[q] = (float *)(b + lay.pdist[q]);
        // (test hook, genpc_fps_defer(2): the check's copy of one recorded minimum is zeroed -- the check must fail)
        if (t_fps_defer == 2 && jobs.k[q] > 8 && hipMemsetAsync(cp.pdist[q] + 8, 0, sizeof(float), st) != hipSuccess) return false;
        cp.verr[q] = (int *)b + q;
        cp.segoff[q] = lay.segoff[q];
    }
    if (hipEventRecord(d->fork[sl], st) != hipSuccess || hipStreamWaitEvent(d->side, d->fork[sl], 0) != hipSuccess) return false;
    launch_verify(cp, nj, false, c.fma, c.cus, d->side, (float *)(b + lay.segmin), d->violations, 0);
    if (hipEventRecord(d->done[sl], d->side) != hipSuccess) return false;
    d->used[sl] = true;
    return true;
}

void fps_deferred_prepare(hipStream_t st)
{
    FpsDeferred *d = fps_deferred_of(st, true);
    if (d) {
        (void)hipEventRecord(d->fork[0], d->side);
        (void)hipStreamSynchronize(d->side);
    }
}

}  // namespace genpc

GENPC_API int genpc_fps_defer(int on)
{
    const int prev = genpc::t_fps_defer;
    genpc::t_fps_defer = on == 2 ? 2 : (on ? 1 : 0);
    return prev;
}

GENPC_API int genpc_fps_deferred_check(void *stream)
{
    using namespace genpc;
    FpsDeferred *d = fps_deferred_of((hipStream_t)stream, false);
    if (!d) return 0;
    int v = 0;
    if (!check(hipStreamSynchronize(d->side), "hipStreamSynchronize(fps check)")) return -1;
    if (!check(hipMemcpy(&v, d->violations, sizeof(int), hipMemcpyDeviceToHost), "hipMemcpy(fps check)")) return -1;
    if (v != 0 && !check(hipMemset(d->violations, 0, sizeof(int)), "hipMemset(fps check)")) return -1;
    return v;
}

// The check on the caller's arrays (tests/test_gpu_fps_check.py): a job table of nj clouds through launch_verify in its in-line
// form, as fps_call.hip's verify_clouds hands it one -- verdict words and segment minima from the scratch pool, a cloud's rows
// of segment minima behind the earlier clouds', the poisoning kernel behind the check.
GENPC_API int genpc_fps_verify_probe(int nj, const int *n, const int *k, const float *const *xyz, int *const *out,
                                     const float *const *pdist, int nseg, int single, void *stream)
{
    using namespace genpc;
    if (nj < 1 || nj > kFMaxJobs) return ragged_refuse("genpc_fps_verify_probe", "need 1 <= nj <= 8 clouds");
    if (!n || !k || !xyz || !out || !pdist) return ragged_refuse("genpc_fps_verify_probe", "a null table");
    if (nseg < 0 || nseg > kFVMaxSeg) return ragged_refuse("genpc_fps_verify_probe", "need 0 <= nseg <= 16");
    size_t points = 0;
    for (int q = 0; q < nj; q++) {
        if (!xyz[q] || !out[q] || !pdist[q]) return ragged_refuse("genpc_fps_verify_probe", "a null array");
        if (k[q] < 1 || k[q] > n[q]) return ragged_refuse("genpc_fps_verify_probe", "need 1 <= k <= n for every cloud");
        points += (size_t)n[q];
    }
    if (points > (size_t)kFpsLargeMaxN) return ragged_refuse("genpc_fps_verify_probe", "more than 4194304 points");
    hipStream_t st = (hipStream_t)stream;
    int *verr; float *segmin;
    WsLayout L;
    L.add(verr, kFMaxJobs);
    L.add(segmin, points * kFVMaxSeg);
    if (!ws_alloc(L, kWsFpsVerifyProbe, st)) return 0;
    if (!check(hipMemsetAsync(verr, 0, kFMaxJobs * sizeof(int), st), "hipMemsetAsync(fps verify probe)")) return 0;
    // the call as fps_call would describe it (the check reads the recorded minima only), and its one job table
    float *pd_of[kFMaxJobs];
    int seg_of[kFMaxJobs];
    size_t seg_off = 0;
    for (int q = 0; q < nj; q++) {
        pd_of[q] = const_cast<float *>(pdist[q]);
        seg_of[q] = (int)seg_off;
        seg_off += (size_t)n[q];
    }
    const FpsCall call = {arith_mode() != 0, num_cus(), st, n, k, xyz, out, pd_of, seg_of, nullptr, verr, segmin};
    FpsJobs jobs = {};
    for (int q = 0; q < nj; q++) fps_fill_job(jobs, q, call, q);
    launch_verify(jobs, nj, single != 0, call.fma, call.cus, call.st, call.segmin, nullptr, nseg);
    return check(hipGetLastError(), "fps verify probe launch") ? 1 : 0;
}
