// fps_call.hip -- the entry points of farthest point sampling (genpc_fps, genpc_fps_multi, genpc_fps_large, genpc_fps_plan,
// genpc_fps_tune, genpc_fps_stats) and the one body behind the sampling calls, fps_call: admit the clouds, ask fps_plan.h for
// every decision, lay out the workspace, run the three samplers (fps_grid.hip, fps_large.hip, fps.hip) on the clouds the plan
// gave each, and have every finished sequence checked (fps_verify.hip).
#include "fps.h"
#include "../../include/genpc_hip.h"
#include <vector>

namespace genpc {

thread_local int t_fps_multi_wg = 0;

// the check of the clouds sel[0 ..) in groups of kFMaxJobs; defer: null = in line
static void verify_clouds(const FpsCall &call, const std::vector<int> &sel, bool single, FpsDeferred *defer)
{
    for (size_t q0 = 0; q0 < sel.size(); q0 += kFMaxJobs) {
        FpsJobs jobs = {};
        int nj = 0;
        for (; nj < kFMaxJobs && q0 + nj < sel.size(); nj++) fps_fill_job(jobs, nj, call, sel[q0 + nj]);
        if (!defer || !fps_verify_deferred(call, jobs, nj, defer)) fps_verify(call, jobs, nj, single);
    }
}

}  // namespace genpc

/* Test hook (applies to the calling host thread; returns the previous setting): 256 = every cloud takes the multi-workgroup
 * kernel (never the one-workgroup kernel of fps_grid.hip), 0 = the default choice; any other value is refused (-1). */
GENPC_API int genpc_fps_tune(int mode)
{
    if (mode != 0 && mode != 256) {
        genpc::set_error("genpc_fps_tune: the mode is 0 or 256");
        return -1;
    }
    const int prev = genpc::t_fps_multi_wg;
    genpc::t_fps_multi_wg = mode;
    return prev;
}

// The body of genpc_fps_multi (force_large = 0: every cloud takes the sampler fps_plan gives it) and of genpc_fps_large (1).
static int fps_call(int c, const int *n, const int *k, const float *const *xyz, int *const *out_idx, void *stream, int force_large)
{
    using namespace genpc;
    if (c <= 0) return 1;
    for (int j = 0; j < c; j++) {
        if (k[j] <= 0 || k[j] > n[j] || fps_plan(n[j], force_large).sampler == kFpsNone) {
            fprintf(stderr, "genpc_fps: need 0 < k <= n <= %d\n", kFpsLargeMaxN);
            set_error("genpc_fps: need 0 < k <= n <= 4194304 for every cloud");
            return -1;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const bool fma = arith_mode() != 0;
    FpsDevice dev;
    if (!fps_device(fma, dev)) return 0;
    // ---- the plan.  Which sampler: clouds that fit one workgroup's LDS take the pruned sampling of fps_grid.hip (no hand-off,
    // several samples per round, updates confined to the ball a sample can change), the others the multi-workgroup kernel of
    // fps.hip.  Same sequences (tests/test_gpu_fps.py runs both on every case); genpc_fps_tune(256): never the former.
    // Clouds beyond the multi-workgroup kernel's registers, and every cloud of genpc_fps_large, take the third sampler
    // (fps_large.hip: one workgroup again, its state in global memory).  A ragged call may mix all three.
    const bool grid_on = t_fps_multi_wg == 0;
    std::vector<int> sampler(c), grid, multi, large;
    for (int j = 0; j < c; j++) {
        const int s = fps_plan(n[j], force_large).sampler;
        sampler[j] = s == kFpsGrid && !grid_on ? (int)kFpsMulti : s;
        (sampler[j] == kFpsGrid ? grid : (sampler[j] == kFpsMulti ? multi : large)).push_back(j);
    }
    // the multi-workgroup clouds: each one's workgroups and points per thread on this device, and the launches they share
    const int cb = (int)multi.size();
    std::vector<FpsShape> shape(cb);
    for (int q = 0; q < cb; q++) {
        shape[q] = fps_multi_shape(n[multi[q]], dev);
        if (!shape[q].ok) {
            set_error("genpc_fps: the cloud needs more co-resident workgroups than the device admits");
            return 0;
        }
    }
    std::vector<FpsLaunch> launches(cb);
    std::vector<int> slot0(cb);
    const int nl = fps_multi_launches(cb, shape.data(), dev, launches.data(), slot0.data());
    // ---- the workspace
    const FpsWorkspace w = fps_workspace(c, n, k, sampler.data(), cb, shape.data());
    int *err, *verr; char *slots; float *pdist, *segmin; float4 *spt;
    float4 *lspt; unsigned *ldmin, *lchmax; int *lstart; CellGridHdr *lhdr;
    WsLayout L;
    L.add(err, 64);          // the 256-byte status block: [0] error, [1 ..] the clouds' hand-off rounds (genpc_fps_stats reads them back)
    static_assert(kFpsSlotBytes == 128, "two slots per workgroup (w.slots is even) are whole 256-byte lines: add() reserves what was reserved unrounded before");
    L.add(slots, w.slots * kFpsSlotBytes);
    L.add(verr, c);
    L.add(pdist, w.k_pad);
    L.add(segmin, w.seg_points * kFVMaxSeg);
    L.add(spt, w.grid_points);
    // the large sampler's pieces, as fps_plan counts them (none for a call without such a cloud)
    L.add(lspt, w.large_points);
    L.add(ldmin, w.large_points);
    L.add(lchmax, w.large_chunks);
    L.add(lstart, w.large_starts);
    L.add(lhdr, w.large_clouds);
    if (!ws_alloc(L, kWsFps, st)) return 0;
    if (!check(hipMemsetAsync(err, 0, (size_t)((char *)pdist - (char *)err), st), "hipMemsetAsync(fps)")) return 0;
    std::vector<float *> pd_of(c);
    std::vector<int> seg_of(c);
    size_t pd_off = 0, seg_off = 0;
    for (int j = 0; j < c; j++) {
        pd_of[j] = pdist + pd_off;
        seg_of[j] = (int)seg_off;
        pd_off += fps_k_pad(k[j]);
        seg_off += fps_seg_points(n[j], sampler[j]);
    }
    const FpsCall call = {fma, dev.cus, st, n, k, xyz, out_idx, pd_of.data(), seg_of.data(), err, verr, segmin};
    // ---- the three samplers, each followed by the check of its clouds
    FpsDeferred *defer = t_fps_defer ? fps_deferred_of(st, true) : nullptr;
    if (!grid.empty()) {
        if (fps_grid_run(fma, (int)grid.size(), grid.data(), n, k, xyz, out_idx, pd_of.data(), spt, err, st) != 1) return 0;
        verify_clouds(call, grid, false, defer);
    }
    if (!large.empty()) {
        if (fps_large_run(fma, (int)large.size(), large.data(), n, k, xyz, out_idx, pd_of.data(), lspt, ldmin, lchmax, lstart, lhdr, err, st) != 1)
            return 0;
        verify_clouds(call, large, true, nullptr);          // (always in line: genpc_fps_defer defers the LDS kernel's checks only)
    }
    if (fps_multi_run(call, multi.data(), shape.data(), nl, launches.data(), slot0.data(), slots) != 1) return 0;
    if (!check(hipGetLastError(), "fps launch")) return 0;
    return 1;
}

GENPC_API int genpc_fps_multi(int c, const int *n, const int *k, const float *const *xyz, int *const *out_idx, void *stream)
{
    return fps_call(c, n, k, xyz, out_idx, stream, 0);
}

GENPC_API int genpc_fps_large(int c, const int *n, const int *k, const float *const *xyz, int *const *out_idx, void *stream)
{
    return fps_call(c, n, k, xyz, out_idx, stream, 1);
}

GENPC_API int genpc_fps_plan(int n, int force_large, int out[8])
{
    if (!out) return -1;
    const genpc::FpsPlan p = genpc::fps_plan(n, force_large);
    out[0] = p.sampler; out[1] = p.cells_max; out[2] = p.cells_target; out[3] = p.npad;
    out[4] = p.chunks; out[5] = p.starts; out[6] = p.lds_bytes; out[7] = p.build_own;
    return p.sampler == genpc::kFpsNone ? -1 : 1;
}

GENPC_API int genpc_fps_stats(int c, int *rounds, void *stream)
{
    // exchanges (hand-off rounds) each of the first c <= 32 clouds of the last genpc_fps_multi call on this
    // stream took; synchronises the stream
    using namespace genpc;
    if (c < 0 || c > 60) return -1;
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace(kWsFps, 256, st);
    if (!ws) return 0;
    if (!check(hipMemcpyAsync(rounds, ws + 4, (size_t)c * sizeof(int), hipMemcpyDeviceToHost, st), "fps stats copy")) return 0;
    return check(hipStreamSynchronize(st), "fps stats sync") ? 1 : 0;
}

GENPC_API int genpc_fps(int c, int n, const float *xyz, int k, int *out_idx, void *stream)
{
    if (c <= 0 || k <= 0) return 1;
    // C clouds of one size: chunks of kFMaxJobs through the ragged entry
    for (int c0 = 0; c0 < c; c0 += genpc::kFMaxJobs) {
        const int cc = c - c0 < genpc::kFMaxJobs ? c - c0 : genpc::kFMaxJobs;
        int ns[genpc::kFMaxJobs], ks[genpc::kFMaxJobs];
        const float *xs[genpc::kFMaxJobs];
        int *os[genpc::kFMaxJobs];
        for (int j = 0; j < cc; j++) {
            ns[j] = n; ks[j] = k;
            xs[j] = xyz + (size_t)(c0 + j) * n * 3;
            os[j] = out_idx + (size_t)(c0 + j) * k;
        }
        const int rc = genpc_fps_multi(cc, ns, ks, xs, os, stream);
        if (rc != 1) return rc;
    }
    return 1;
}
