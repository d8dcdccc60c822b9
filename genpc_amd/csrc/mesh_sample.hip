// mesh_sample.hip -- area-weighted surface samples of a triangle mesh, every bit a function of (mesh, seed, i).
//
// The definition is stated in include/genpc_hip.h (genpc_mesh_sample) and restated in numpy by tests/mesh_sample_ref.py.
// In short: a face's weight is the INTEGER floor(A_f * 2^(38 - ilogb(Amax))), A_f = |e1 x e2| in fp64 (unfused, root
// correctly rounded), so the cumulative weights are the same in every summation order and the parallel scans below need
// no tolerance; sample i draws Philox4x32-10(counter i, key seed), picks the face by a 64 x 64 -> high 64 multiply against
// the total weight W and the point by trimesh's folded parallelogram on two 24-bit uniforms.
//   * mesh_face_kernel: a lane per face.  The three indices are checked against [0, nv) BEFORE a vertex is loaded and the
//     nine coordinates for finiteness; a failing face raises the header's `bad` word and has area 0.  The areas go to the
//     workspace (the slot that later holds the face's cumulative weight), their maximum through a wave reduction and one
//     atomic max per wave on the bit pattern (positive doubles order as their bits).
//   * mesh_weight_scan_kernel: a workgroup per kMsChunk = 1024 faces, four consecutive faces a lane: weights, the inclusive
//     scan INSIDE the chunk (written over the areas) and the chunk's sum.
//   * mesh_chunk_scan_kernel: one workgroup of 1024 lanes, 16 consecutive chunk sums a lane (nf <= 2^24: at most 16384
//     chunks), scans the sums in place and writes the status word.
//   * mesh_sample_kernel: a lane per sample.  Two searches: the chunk (first chunk whose inclusive sum exceeds t), then the
//     face inside it against t minus the chunks before -- the same face as one search of the global cumulative weights,
//     which are never materialised.  The chunk sums are staged in LDS when there are at most kMsStage = 2048 of them
//     (16 KiB a workgroup: eight workgroups of 256 lanes, the CU's 32-wave limit, take 128 of its 160 KiB, so the staging
//     never costs a wave); larger meshes (nf > 2^21) search them in global memory.
// Everything is enqueued on the caller's stream in the caller's workspace; nothing is read back.
#include "mesh_sample.h"
#include "../../include/genpc_hip.h"

namespace genpc {

constexpr size_t kMsHeaderBytes = 256;

static size_t ms_align(size_t v) { return (v + 255) & ~(size_t)255; }
static size_t ms_chunk_offset(int nf) { return kMsHeaderBytes + ms_align((size_t)nf * sizeof(u64)); }

__global__ __launch_bounds__(kMsBlock) void mesh_face_kernel(int nv, const float *__restrict__ V, int nf, const int *__restrict__ F,
                                                             double *__restrict__ area, MsHeader *__restrict__ hdr)
{
    const int f = blockIdx.x * kMsBlock + threadIdx.x;
    double a = 0.0;
    bool bad = false;
    if (f < nf) {
        a = ms_face_area(nv, V, F, f, bad);
        area[f] = a;
    }
    ms_wave_fold(a, bad, hdr);
}

__global__ __launch_bounds__(kMsBlock) void mesh_weight_scan_kernel(int nf, u64 *__restrict__ cum, const MsHeader *__restrict__ hdr,
                                                                    u64 *__restrict__ chunk_sum)
{
    __shared__ u64 s_w[kMsBlock / kWave];
    ms_weight_scan_chunk(nf, cum, hdr, blockIdx.x, chunk_sum + blockIdx.x, s_w);
}

__global__ __launch_bounds__(kMsScanBlock) void mesh_chunk_scan_kernel(int chunks, u64 *__restrict__ chunk_sum, const MsHeader *__restrict__ hdr,
                                                                       int *__restrict__ out_status)
{
    __shared__ u64 s_w[kMsScanBlock / kWave];
    ms_chunk_scan(chunks, chunk_sum, hdr, out_status, s_w);
}

template <bool STAGED>
__global__ __launch_bounds__(kMsBlock) void mesh_sample_kernel(const float *__restrict__ V, const float *__restrict__ C, int nf,
                                                               const int *__restrict__ F, const u64 *__restrict__ cum,
                                                               const u64 *__restrict__ chunk_sum, int chunks, int count,
                                                               uint32_t seed_lo, uint32_t seed_hi, float *__restrict__ out_xyz,
                                                               float *__restrict__ out_col, int *__restrict__ out_face,
                                                               float *__restrict__ out_bary)
{
    __shared__ u64 s_sum[STAGED ? kMsStage : 1];
    if (STAGED) {
        for (int k = threadIdx.x; k < chunks; k += kMsBlock) s_sum[k] = chunk_sum[k];
        __syncthreads();
    }
    const u64 *sums = STAGED ? s_sum : chunk_sum;
    const int i = blockIdx.x * kMsBlock + threadIdx.x;
    if (i >= count) return;
    ms_draw(V, C, nf, F, cum, sums, chunks, i, seed_lo, seed_hi, out_xyz, out_col, out_face, out_bary);
}

}  // namespace genpc

GENPC_API int genpc_mesh_sample_bytes(int nf)
{
    using namespace genpc;
    if (nf < 1 || nf > kMsMaxFaces) {
        set_error("genpc_mesh_sample_bytes: nf must be in [1, 2^24]");
        return -1;
    }
    return (int)(ms_chunk_offset(nf) + ms_align((size_t)ceil_div(nf, kMsChunk) * sizeof(u64)));      // < 2^28
}

GENPC_API int genpc_mesh_sample(int nv, const float *vertices, const float *vertex_colors, int nf, const int *faces, int count,
                                unsigned long long seed, float *out_xyz, float *out_colors, int *out_face, float *out_bary,
                                int *out_status, void *ws, void *stream)
{
    using namespace genpc;
    if (nf < 1 || nf > kMsMaxFaces || count < 1 || nv < 1) {
        set_error("genpc_mesh_sample: nv >= 1, 1 <= nf <= 2^24 and count >= 1 are required");
        return -1;
    }
    if (out_colors && !vertex_colors) {
        set_error("genpc_mesh_sample: out_colors without vertex_colors");
        return -1;
    }
    if (!vertices || !faces || !out_xyz || !out_status || !ws) {
        set_error("genpc_mesh_sample: null pointer");
        return -1;
    }
    hipStream_t st = (hipStream_t)stream;
    const int chunks = ceil_div(nf, kMsChunk);
    MsHeader *hdr = (MsHeader *)ws;
    u64 *cum = (u64 *)((char *)ws + kMsHeaderBytes);
    u64 *chunk_sum = (u64 *)((char *)ws + ms_chunk_offset(nf));
    if (!check(hipMemsetAsync(hdr, 0, kMsHeaderBytes, st), "genpc_mesh_sample header memset")) return -1;
    hipLaunchKernelGGL(mesh_face_kernel, dim3(ceil_div(nf, kMsBlock)), dim3(kMsBlock), 0, st, nv, vertices, nf, faces, (double *)cum, hdr);
    if (!check(hipGetLastError(), "mesh_face_kernel launch")) return -1;
    hipLaunchKernelGGL(mesh_weight_scan_kernel, dim3(chunks), dim3(kMsBlock), 0, st, nf, cum, (const MsHeader *)hdr, chunk_sum);
    if (!check(hipGetLastError(), "mesh_weight_scan_kernel launch")) return -1;
    hipLaunchKernelGGL(mesh_chunk_scan_kernel, dim3(1), dim3(kMsScanBlock), 0, st, chunks, chunk_sum, (const MsHeader *)hdr, out_status);
    if (!check(hipGetLastError(), "mesh_chunk_scan_kernel launch")) return -1;
    const dim3 grid(ceil_div(count, kMsBlock));
    if (chunks <= kMsStage)
        hipLaunchKernelGGL(mesh_sample_kernel<true>, grid, dim3(kMsBlock), 0, st, vertices, vertex_colors, nf, faces, (const u64 *)cum,
                           (const u64 *)chunk_sum, chunks, count, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), out_xyz,
                           out_colors, out_face, out_bary);
    else
        hipLaunchKernelGGL(mesh_sample_kernel<false>, grid, dim3(kMsBlock), 0, st, vertices, vertex_colors, nf, faces, (const u64 *)cum,
                           (const u64 *)chunk_sum, chunks, count, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), out_xyz,
                           out_colors, out_face, out_bary);
    return check(hipGetLastError(), "mesh_sample_kernel launch") ? 1 : -1;
}
