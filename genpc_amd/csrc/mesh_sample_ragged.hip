// mesh_sample_ragged.hip -- genpc_mesh_sample over a ragged batch: c meshes of any sizes, packed, each with its own seed and
// sample count, one call.  Mesh j's samples are the bits of genpc_mesh_sample on that mesh alone with seeds[j]: the definition
// is include/genpc_hip.h's (genpc_mesh_sample), the device bodies are mesh_sample.h's, shared with mesh_sample.hip; Amax, the
// weight shift, the cumulative weights and the status are per mesh, sample i of a mesh uses Philox counter i.
//
// The tables ride BY VALUE in the kernel arguments and the workgroups are numbered by mesh_sample_ragged_plan.h: a chunk of
// 1024 faces never spans two meshes, a workgroup of the sampling launch serves one mesh.  A memset of the headers and FOUR
// launches, whatever c is:
//   mesh_ragged_face_kernel         a workgroup per chunk item, four faces a lane (strided by the workgroup: coalesced).  A face
//                                   index is checked against its OWN mesh's nv before anything is loaded through it.  Areas to the
//                                   scratch, the mesh's maximum and its `bad` word through one integer atomic max / or per wave.
//   mesh_ragged_weight_scan_kernel  a workgroup per chunk item: weights, the scan inside the chunk, the chunk's sum to its slot
//   mesh_ragged_chunk_scan_kernel   a workgroup per mesh: scans the mesh's chunk sums in place, writes out_status[j]
//   mesh_ragged_sample_kernel       a workgroup per 256 samples of one mesh; the mesh's chunk sums are staged in LDS when there are
//                                   at most kMsStage = 2048 of them, larger meshes (nf > 2^21) search them in global memory -- a
//                                   branch uniform over the workgroup, each side with its own address space
// Integer atomics only, no spin, no hand-off between workgroups: the same bits on every run.  Nothing is read back; scratch
// is one block of the pool (kWsMeshSampleRagged).
#include "mesh_sample.h"
#include "mesh_sample_ragged_plan.h"
#include "../../include/genpc_hip.h"

namespace genpc {

static_assert(kMsRaggedMaxMeshes == GENPC_MESH_SAMPLE_RAGGED_MAX_MESHES, "the header names the bound");
static_assert((1 << kMsRaggedChunkShift) == kMsChunk && (1 << kMsRaggedSampleShift) == kMsBlock, "the plan's items are the kernels' workgroups");
static_assert(kMsRaggedMaxFaces == kMsMaxFaces, "one workgroup scans a mesh's chunk sums");
static_assert(sizeof(MsRaggedHeader) == sizeof(MsHeader), "the plan sizes the headers");

__global__ __launch_bounds__(kMsBlock) void mesh_ragged_face_kernel(MsRaggedTable t, const float *__restrict__ V, const int *__restrict__ F,
                                                                    double *__restrict__ area, MsHeader *__restrict__ hdr)
{
    const int item = blockIdx.x;
    const int mesh = ms_ragged_mesh_of(t.foff, t.c, item, kMsRaggedChunkShift);
    const int f0 = t.foff[mesh], nf = t.foff[mesh + 1] - f0;
    const int v0 = t.voff[mesh], nv = t.voff[mesh + 1] - v0;
    const int base = ms_ragged_item_base(t.foff, mesh, item, kMsRaggedChunkShift);
    if (base >= nf) return;                                         // (uniform: the whole workgroup leaves)
    double a = 0.0;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < kMsChunk / kMsBlock; k++) {
        const int f = base + k * kMsBlock + threadIdx.x;
        if (f < nf) {
            const double x = ms_face_area(nv, V + (size_t)v0 * 3, F + (size_t)f0 * 3, f, bad);
            area[(size_t)f0 + f] = x;
            a = fmax(a, x);
        }
    }
    ms_wave_fold(a, bad, hdr + mesh);
}

__global__ __launch_bounds__(kMsBlock) void mesh_ragged_weight_scan_kernel(MsRaggedTable t, u64 *__restrict__ cum,
                                                                           const MsHeader *__restrict__ hdr, u64 *__restrict__ chunk_sum)
{
    __shared__ u64 s_w[kMsBlock / kWave];
    const int item = blockIdx.x;
    const int mesh = ms_ragged_mesh_of(t.foff, t.c, item, kMsRaggedChunkShift);
    const int f0 = t.foff[mesh], nf = t.foff[mesh + 1] - f0;
    const int chunk = item - ms_ragged_first_item(t.foff, mesh, kMsRaggedChunkShift);
    if (chunk * kMsChunk >= nf) return;                             // (uniform; the idle item's slot is never read)
    ms_weight_scan_chunk(nf, cum + f0, hdr + mesh, chunk, chunk_sum + item, s_w);
}

__global__ __launch_bounds__(kMsScanBlock) void mesh_ragged_chunk_scan_kernel(MsRaggedTable t, u64 *__restrict__ chunk_sum,
                                                                              const MsHeader *__restrict__ hdr, int *__restrict__ out_status)
{
    __shared__ u64 s_w[kMsScanBlock / kWave];
    const int mesh = blockIdx.x;
    const int nf = t.foff[mesh + 1] - t.foff[mesh];
    ms_chunk_scan((nf + kMsChunk - 1) / kMsChunk, chunk_sum + ms_ragged_first_item(t.foff, mesh, kMsRaggedChunkShift), hdr + mesh,
                  out_status + mesh, s_w);
}

__global__ __launch_bounds__(kMsBlock) void mesh_ragged_sample_kernel(MsRaggedTable t, const float *__restrict__ V, const float *__restrict__ C,
                                                                      const int *__restrict__ F, const u64 *__restrict__ cum,
                                                                      const u64 *__restrict__ chunk_sum, float *__restrict__ out_xyz,
                                                                      float *__restrict__ out_col, int *__restrict__ out_face,
                                                                      float *__restrict__ out_bary)
{
    __shared__ u64 s_sum[kMsStage];
    const int item = blockIdx.x;
    const int mesh = ms_ragged_mesh_of(t.soff, t.c, item, kMsRaggedSampleShift);
    const int s0 = t.soff[mesh], count = t.soff[mesh + 1] - s0;
    const int base = ms_ragged_item_base(t.soff, mesh, item, kMsRaggedSampleShift);
    if (base >= count) return;                                      // (uniform: the whole workgroup leaves)
    const int f0 = t.foff[mesh], nf = t.foff[mesh + 1] - f0;
    const size_t v0 = (size_t)t.voff[mesh];
    const int chunks = (nf + kMsChunk - 1) / kMsChunk;
    const u64 *sums = chunk_sum + ms_ragged_first_item(t.foff, mesh, kMsRaggedChunkShift);
    const uint32_t seed_lo = (uint32_t)(t.seed[mesh] & 0xffffffffu), seed_hi = (uint32_t)(t.seed[mesh] >> 32);
    // everything below sees the mesh alone: its vertices, faces, weights and output rows
    V += v0 * 3;
    if (C) C += v0 * 3;
    F += (size_t)f0 * 3;
    cum += f0;
    out_xyz += (size_t)s0 * 3;
    if (out_col) out_col += (size_t)s0 * 3;
    if (out_face) out_face += s0;
    if (out_bary) out_bary += (size_t)s0 * 3;
    const int i = base + threadIdx.x;
    if (chunks <= kMsStage) {
        for (int k = threadIdx.x; k < chunks; k += kMsBlock) s_sum[k] = sums[k];
        __syncthreads();
        if (i < count) ms_draw(V, C, nf, F, cum, s_sum, chunks, i, seed_lo, seed_hi, out_xyz, out_col, out_face, out_bary);
    } else {
        if (i < count) ms_draw(V, C, nf, F, cum, sums, chunks, i, seed_lo, seed_hi, out_xyz, out_col, out_face, out_bary);
    }
}

}  // namespace genpc

GENPC_API int genpc_mesh_sample_ragged(int c, const int *voff, const int *foff, const int *soff, const unsigned long long *seeds,
                                       const float *vertices, const float *vertex_colors, const int *faces, float *out_xyz,
                                       float *out_colors, int *out_face, float *out_bary, int *out_status, void *stream)
{
    using namespace genpc;
    const char *fn = "genpc_mesh_sample_ragged";
    // every refusal is decided here, before anything touches a device
    MsRaggedTable t;
    const char *err = nullptr;
    const int work = ms_ragged_fill(c, voff, foff, soff, seeds, t, &err);
    if (work < 0) return ragged_refuse(fn, err);
    if (work == 0) return 1;
    if (out_colors && !vertex_colors) return ragged_refuse(fn, "out_colors without vertex_colors");
    if (!vertices || !faces || !out_status || (t.soff[c] > 0 && !out_xyz)) return ragged_refuse(fn, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    WsLayout L;
    MsRaggedScratch s;
    ms_ragged_layout(t, L, s);
    if (!ws_alloc(L, kWsMeshSampleRagged, st)) return -1;
    MsHeader *hdr = (MsHeader *)s.hdr;
    if (!check(hipMemsetAsync(hdr, 0, (size_t)c * sizeof(MsHeader), st), "genpc_mesh_sample_ragged header memset")) return -1;
    const int chunk_items = ms_ragged_first_item(t.foff, c, kMsRaggedChunkShift);
    const int sample_items = ms_ragged_first_item(t.soff, c, kMsRaggedSampleShift);
    hipLaunchKernelGGL(mesh_ragged_face_kernel, dim3(chunk_items), dim3(kMsBlock), 0, st, t, vertices, faces, (double *)s.cum, hdr);
    if (!check(hipGetLastError(), "mesh_ragged_face_kernel launch")) return -1;
    hipLaunchKernelGGL(mesh_ragged_weight_scan_kernel, dim3(chunk_items), dim3(kMsBlock), 0, st, t, s.cum, (const MsHeader *)hdr, s.chunk_sum);
    if (!check(hipGetLastError(), "mesh_ragged_weight_scan_kernel launch")) return -1;
    hipLaunchKernelGGL(mesh_ragged_chunk_scan_kernel, dim3(c), dim3(kMsScanBlock), 0, st, t, s.chunk_sum, (const MsHeader *)hdr, out_status);
    if (!check(hipGetLastError(), "mesh_ragged_chunk_scan_kernel launch")) return -1;
    // (every mesh owns at least one sample item, so the grid is never empty; a mesh with count 0 has its idle item alone)
    hipLaunchKernelGGL(mesh_ragged_sample_kernel, dim3(sample_items), dim3(kMsBlock), 0, st, t, vertices, vertex_colors, faces,
                       (const u64 *)s.cum, (const u64 *)s.chunk_sum, out_xyz, out_colors, out_face, out_bary);
    return check(hipGetLastError(), "mesh_ragged_sample_kernel launch") ? 1 : -1;
}
