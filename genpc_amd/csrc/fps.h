// fps.h -- what the farthest-point-sampling files share (fps_call.hip: the entry points and the call; fps_grid.hip, fps.hip,
// fps_large.hip: the three samplers; fps_verify.hip: the check of a finished sequence, in line or deferred): the job table of a
// launch, the call as the passes see it, the samplers' and the verification's host functions and the per-thread hooks.
// Every host decision of a call is fps_plan.h's.
#pragma once
#include "emd.h"          // persist_reserve, persist_commit, emd_auction_capacity
#include "fps_plan.h"

namespace genpc {

static_assert(WsLayout::up(1) == kFpsWsAlign && WsLayout::up(kFpsWsAlign) == kFpsWsAlign && WsLayout::up(kFpsWsAlign + 1) == 2 * kFpsWsAlign,
              "fps_plan.h rounds by the scratch pool's rule");

// The clouds of one launch of fps_kernel or of one verification
struct FpsJobs {
    const float *xyz[kFMaxJobs];
    int *out[kFMaxJobs];
    int n[kFMaxJobs], k[kFMaxJobs], W[kFMaxJobs];
    int slot0[kFMaxJobs];        // first slot of the job in the slot array (slots are per (job, parity, workgroup))
    int stat0;                   // index of the launch's first cloud in the call (statistics)
    float *pdist[kFMaxJobs];     // the running minimum of every sample when it was drawn (fps_verify_kernel)
    int *verr[kFMaxJobs];        // != 0: the verification found a step whose sample is not the first arg-max
    int segoff[kFMaxJobs];       // first point of the job in the verification's per-(point, segment) minima
};

// One call's arguments and the pieces fps_call carved for it; the arrays have an entry per cloud of the call
struct FpsCall {
    bool fma;
    int cus;
    hipStream_t st;
    const int *n, *k;
    const float *const *xyz;
    int *const *out;
    float *const *pdist;         // where the cloud's recorded minima go
    const int *segoff;           // its first point in segmin
    int *err, *verr;             // the status block ([0] error, [1 ..] the clouds' rounds: genpc_fps_stats); a verdict word per cloud
    float *segmin;
};
// cloud j of the call as entry q of a job table (W and slot0 are the multi-workgroup sampler's to add)
inline void fps_fill_job(FpsJobs &jobs, int q, const FpsCall &c, int j)
{
    jobs.xyz[q] = c.xyz[j];
    jobs.out[q] = c.out[j];
    jobs.pdist[q] = c.pdist[j];
    jobs.verr[q] = c.verr + j;
    jobs.segoff[q] = c.segoff[j];
    jobs.n[q] = c.n[j];
    jobs.k[q] = c.k[j];
}

// ---- the samplers: clouds `sel[0 .. )` (indices into the call's arrays) through one of them; 1, or 0 after a recorded error
// fps_grid.hip: one workgroup per cloud, spatial pruning, running minima in LDS
bool fps_grid_takes(int n);
int fps_grid_run(bool fma, int c, const int *sel, const int *n, const int *k, const float *const *xyz, int *const *out_idx,
                 float *const *pdist_of, float4 *spt, int *err, hipStream_t st);
// fps_large.hip: one workgroup per cloud, spatial pruning, running minima in global memory
int fps_large_run(bool fma, int c, const int *sel, const int *n, const int *k, const float *const *xyz, int *const *out_idx,
                  float *const *pdist_of, float4 *spt, unsigned *dmin, unsigned *chmax, int *start, CellGridHdr *hdr, int *err,
                  hipStream_t st);
// fps.hip: the multi-workgroup kernel.  The device as fps_plan.h wants it (false: a recorded error), and the plan's launches
// carried out -- admission, launch, the check in line.  shape, slot0: per selected cloud; slots: kFpsSlotBytes each.
constexpr size_t kFpsSlotBytes = 128;
bool fps_device(bool fma, FpsDevice &dev);
int fps_multi_run(const FpsCall &c, const int *sel, const FpsShape *shape, int nl, const FpsLaunch *launches, const int *slot0, void *slots);

// ---- fps_verify.hip: a group of up to kFMaxJobs sampled clouds against the definition, whichever kernel sampled them.
// single: never cut into segments (fps_verify_segments).  In line: behind the sampling on the call's stream, a failed check
// poisons out[0].  Deferred (genpc_fps_defer; d from fps_deferred_of): on copies, on the side stream, a failed check is counted;
// false: not possible now, the caller checks in line.
struct FpsDeferred;
FpsDeferred *fps_deferred_of(hipStream_t st, bool create);
void fps_deferred_prepare(hipStream_t st);          // (pose.hip genpc_streams_prepare: the side stream made and first used ahead of the caller's other streams)
void fps_verify(const FpsCall &c, const FpsJobs &jobs, int nj, bool single);
bool fps_verify_deferred(const FpsCall &c, const FpsJobs &jobs, int nj, FpsDeferred *d);

// the per-thread hooks: genpc_fps_tune (t_fps_multi_wg, common.h) and genpc_fps_defer
extern thread_local int t_fps_defer;

}  // namespace genpc
