// pose_ragged.hip -- the two kernels a ragged alignment call (pose.hip genpc_pose_optimize_ragged, genpc_pose_loss_grad_ragged) has
// beside the loop's own: the one that puts the element tables on the device, and the packed replication of the clouds per start.
// Every per-point kernel of the loop is the equal-size loop's, given a table (pose.h pose_span); the shape of the call is
// pose_ragged_plan.h's.
//   pose_ragged_tables_kernel      the element tables travel BY VALUE in this launch's arguments (ragged_table.h's way: no copy is
//                                  enqueued that could stall the stream, nothing of the caller's host arrays is read after the entry
//                                  point returns) and are written to scratch, where the loop's kernels read them with scalar loads
//   pose_ragged_replicate_kernel   element scan * starts + start gets scan's clouds (and colours): dst is packed by the element
//                                  tables, i.e. scan j's copies start at starts * off[j] and lie n_j apart
#include "pose.h"

namespace genpc {

struct PoseRaggedTablesArgs {
    RaggedTable t;             // qoff: the complete clouds' element table, toff: the partial clouds'
    int *coff, *poff;          // [t.c + 1] each
};
static_assert(sizeof(PoseRaggedTablesArgs) <= 4096, "the element tables must fit the kernel arguments");

__global__ __launch_bounds__(kQBlock) void pose_ragged_tables_kernel(PoseRaggedTablesArgs a)
{
    const int i = blockIdx.x * kQBlock + threadIdx.x;
    if (i > a.t.c) return;
    a.coff[i] = a.t.qoff[i];
    a.poff[i] = a.t.toff[i];
}

struct PoseRaggedReplicateArgs {
    RaggedTable t;             // per SCAN: qoff the complete clouds, toff the partial clouds
    int starts;
    const float *src[4];       // complete, partial, complete colours, partial colours (null: absent)
    float *dst[4];
};
static_assert(sizeof(PoseRaggedReplicateArgs) <= 4096, "the scan tables must fit the kernel arguments");

// grid (width for the largest cloud's 3 n floats, scans)
__global__ __launch_bounds__(kQBlock) void pose_ragged_replicate_kernel(PoseRaggedReplicateArgs a)
{
    const int g = blockIdx.y;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (!a.src[k]) continue;
        const int *off = (k & 1) ? a.t.toff : a.t.qoff;
        const int o = off[g], n = off[g + 1] - o;
        const size_t count = (size_t)n * 3;
        const float *__restrict__ src = a.src[k] + (size_t)o * 3;
        float *__restrict__ dst = a.dst[k] + (size_t)a.starts * o * 3;
        for (size_t j = (size_t)blockIdx.x * kQBlock + threadIdx.x; j < count; j += (size_t)gridDim.x * kQBlock) {
            const float v = src[j];
            for (int r = 0; r < a.starts; r++) dst[(size_t)r * count + j] = v;
        }
    }
}

int pose_ragged_tables(const RaggedTable &elements, int *coff_e, int *poff_e, hipStream_t st)
{
    PoseRaggedTablesArgs a{};
    a.t = elements; a.coff = coff_e; a.poff = poff_e;
    hipLaunchKernelGGL(pose_ragged_tables_kernel, dim3(ceil_div(elements.c + 1, kQBlock)), dim3(kQBlock), 0, st, a);
    return check(hipGetLastError(), "pose_ragged_tables_kernel launch") ? 1 : 0;
}

int pose_ragged_replicate(const RaggedTable &scans, int starts, int width, const float *const src[4], float *const dst[4], hipStream_t st)
{
    PoseRaggedReplicateArgs a{};
    a.t = scans; a.starts = starts;
    for (int k = 0; k < 4; k++) { a.src[k] = src[k]; a.dst[k] = dst[k]; }
    hipLaunchKernelGGL(pose_ragged_replicate_kernel, dim3(width, scans.c), dim3(kQBlock), 0, st, a);
    return check(hipGetLastError(), "pose_ragged_replicate_kernel launch") ? 1 : 0;
}

}  // namespace genpc
