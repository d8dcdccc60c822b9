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
#include "common.h"
#include "../../include/genpc_hip.h"

namespace genpc {

constexpr int kMsBlock = 256;
constexpr int kMsChunk = 1024;                    // faces per scan workgroup: kMsBlock lanes x 4
constexpr int kMsMaxFaces = 1 << 24;
constexpr int kMsScanBlock = 1024;                // the one workgroup that scans the chunk sums,
constexpr int kMsScanPerLane = 16;                // 16 a lane: kMsMaxFaces / kMsChunk = 16384 sums
constexpr int kMsStage = 2048;                    // chunk sums staged in LDS by the sampling kernel
constexpr size_t kMsHeaderBytes = 256;
typedef unsigned long long u64;

struct MsHeader {                                 // zeroed at the head of every call
    u64 amax_bits;                                // max_f A_f as its bit pattern
    int bad;                                      // a face with an index outside [0, nv) or a non-finite vertex
};

static size_t ms_align(size_t v) { return (v + 255) & ~(size_t)255; }
static size_t ms_chunk_offset(int nf) { return kMsHeaderBytes + ms_align((size_t)nf * sizeof(u64)); }

// inclusive prefix sum over the wave's lanes (all 64 active)
__device__ __forceinline__ u64 ms_wave_scan(u64 x)
{
    const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const u64 y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    return x;
}

// the workgroup's exclusive prefix of `total` (one value a lane), WAVES waves; s_w: WAVES words of LDS
template <int WAVES>
__device__ __forceinline__ u64 ms_block_excl(u64 total, u64 *s_w)
{
    const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    const u64 incl = ms_wave_scan(total);
    if (lane == kWave - 1) s_w[wave] = incl;
    __syncthreads();
    u64 before = 0;
    for (int w = 0; w < wave; w++) before += s_w[w];
    return before + (incl - total);
}

__global__ __launch_bounds__(kMsBlock) void mesh_face_kernel(int nv, const float *__restrict__ V, int nf, const int *__restrict__ F,
                                                             double *__restrict__ area, MsHeader *__restrict__ hdr)
{
    const int f = blockIdx.x * kMsBlock + threadIdx.x;
    double a = 0.0;
    bool bad = false;
    if (f < nf) {
        const int i0 = F[(size_t)f * 3 + 0], i1 = F[(size_t)f * 3 + 1], i2 = F[(size_t)f * 3 + 2];
        if ((unsigned)i0 >= (unsigned)nv || (unsigned)i1 >= (unsigned)nv || (unsigned)i2 >= (unsigned)nv) {
            bad = true;                                              // nothing is loaded through a bad index
        } else {
            float p[9];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                p[k] = V[(size_t)i0 * 3 + k];
                p[3 + k] = V[(size_t)i1 * 3 + k];
                p[6 + k] = V[(size_t)i2 * 3 + k];
            }
            bool fin = true;
#pragma unroll
            for (int k = 0; k < 9; k++) fin = fin && (fabsf(p[k]) <= 3.402823466e38f);     // false for NaN and infinity
            if (!fin) {
                bad = true;
            } else {
                const double e1x = __dsub_rn((double)p[3], (double)p[0]), e1y = __dsub_rn((double)p[4], (double)p[1]),
                             e1z = __dsub_rn((double)p[5], (double)p[2]);
                const double e2x = __dsub_rn((double)p[6], (double)p[0]), e2y = __dsub_rn((double)p[7], (double)p[1]),
                             e2z = __dsub_rn((double)p[8], (double)p[2]);
                const double cx = __dsub_rn(__dmul_rn(e1y, e2z), __dmul_rn(e1z, e2y));
                const double cy = __dsub_rn(__dmul_rn(e1z, e2x), __dmul_rn(e1x, e2z));
                const double cz = __dsub_rn(__dmul_rn(e1x, e2y), __dmul_rn(e1y, e2x));
                const double s = __dadd_rn(__dadd_rn(__dmul_rn(cx, cx), __dmul_rn(cy, cy)), __dmul_rn(cz, cz));
                a = __dsqrt_rn(s);                                   // finite: fp32 coordinates cannot overflow an fp64 s
            }
        }
        area[f] = a;
    }
    // the wave's maximum (areas are >= 0 and never NaN) and whether any of its faces failed
    double m = a;
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) m = fmax(m, __shfl_xor(m, d));
    const bool any_bad = __ballot(bad) != 0;
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (m > 0.0) atomicMax(&hdr->amax_bits, (u64)__double_as_longlong(m));
        if (any_bad) atomicOr(&hdr->bad, 1);
    }
}

__global__ __launch_bounds__(kMsBlock) void mesh_weight_scan_kernel(int nf, u64 *__restrict__ cum, const MsHeader *__restrict__ hdr,
                                                                    u64 *__restrict__ chunk_sum)
{
    __shared__ u64 s_w[kMsBlock / kWave];
    const u64 amax_bits = hdr->amax_bits;
    // Amax is 0 (every weight 0) or a normal double (>= 2^-596 for fp32 coordinates): ilogb is its exponent field
    const int shift = amax_bits ? 38 - ((int)(amax_bits >> 52) - 1023) : 0;
    const int base = blockIdx.x * kMsChunk + threadIdx.x * 4;
    u64 w[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int f = base + k;
        // A_f <= Amax: the scaled area is below 2^39, the conversion truncates (= floor, it is >= 0)
        w[k] = f < nf ? (u64)ldexp(__longlong_as_double((long long)cum[f]), shift) : 0;
    }
    w[1] += w[0];
    w[2] += w[1];
    w[3] += w[2];
    const u64 before = ms_block_excl<kMsBlock / kWave>(w[3], s_w);
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (base + k < nf) cum[base + k] = before + w[k];
    if (threadIdx.x == kMsBlock - 1) chunk_sum[blockIdx.x] = before + w[3];
}

__global__ __launch_bounds__(kMsScanBlock) void mesh_chunk_scan_kernel(int chunks, u64 *__restrict__ chunk_sum, const MsHeader *__restrict__ hdr,
                                                                       int *__restrict__ out_status)
{
    __shared__ u64 s_w[kMsScanBlock / kWave];
    const int base = threadIdx.x * kMsScanPerLane;
    u64 v[kMsScanPerLane];
#pragma unroll
    for (int k = 0; k < kMsScanPerLane; k++) {
        v[k] = base + k < chunks ? chunk_sum[base + k] : 0;
        if (k) v[k] += v[k - 1];
    }
    const u64 before = ms_block_excl<kMsScanBlock / kWave>(v[kMsScanPerLane - 1], s_w);
#pragma unroll
    for (int k = 0; k < kMsScanPerLane; k++)
        if (base + k < chunks) chunk_sum[base + k] = before + v[k];
    if (threadIdx.x == kMsScanBlock - 1) *out_status = (hdr->bad || before + v[kMsScanPerLane - 1] == 0) ? -1 : 1;
}

struct Philox4 {
    uint32_t x0, x1, x2, x3;
};

// Philox4x32-10 (Salmon et al., SC'11): counter (c0, c1, 0, 0), key (k0, k1)
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1)
{
    uint32_t c2 = 0, c3 = 0;
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{c0, c1, c2, c3};
}

// first index of a[0, n) whose value exceeds t; the caller guarantees a[n - 1] > t, so the result is in [0, n)
__device__ __forceinline__ int ms_first_above(const u64 *a, int n, u64 t)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    return lo;
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
    const u64 W = sums[chunks - 1];
    if (W == 0) {                                     // status -1: no face can be drawn; the outputs are written all the same
#pragma unroll
        for (int k = 0; k < 3; k++) {
            out_xyz[(size_t)i * 3 + k] = 0.0f;
            if (out_col) out_col[(size_t)i * 3 + k] = 0.0f;
            if (out_bary) out_bary[(size_t)i * 3 + k] = 0.0f;
        }
        if (out_face) out_face[i] = -1;
        return;
    }
    const Philox4 x = philox4x32_10((uint32_t)i, 0u, seed_lo, seed_hi);
    const u64 t = __umul64hi((u64)x.x0 | ((u64)x.x1 << 32), W);           // < W
    // t < W = sums[chunks - 1]; inside chunk c, t - (sums before c) < the chunk's own sum = its last inclusive weight
    const int c = ms_first_above(sums, chunks, t);
    const u64 tl = t - (c ? sums[c - 1] : 0);
    const int f0 = c * kMsChunk;
    const int f = f0 + ms_first_above(cum + f0, min(kMsChunk, nf - f0), tl);
    // cum[f] > tl >= cum[f - 1]: the face has a positive weight, so it passed mesh_face_kernel's checks
    float r1 = (float)(x.x2 >> 8) * 0x1p-24f, r2 = (float)(x.x3 >> 8) * 0x1p-24f;
    if (__fadd_rn(r1, r2) > 1.0f) {
        r1 = __fsub_rn(1.0f, r1);
        r2 = __fsub_rn(1.0f, r2);
    }
    const float b0 = __fsub_rn(__fsub_rn(1.0f, r1), r2);
    const int i0 = F[(size_t)f * 3 + 0], i1 = F[(size_t)f * 3 + 1], i2 = F[(size_t)f * 3 + 2];
    const double d1 = (double)r1, d2 = (double)r2;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double v0 = (double)V[(size_t)i0 * 3 + k], v1 = (double)V[(size_t)i1 * 3 + k], v2 = (double)V[(size_t)i2 * 3 + k];
        const double e1 = __dsub_rn(v1, v0), e2 = __dsub_rn(v2, v0);
        out_xyz[(size_t)i * 3 + k] = (float)__dadd_rn(__dadd_rn(v0, __dmul_rn(e1, d1)), __dmul_rn(e2, d2));
    }
    if (out_col) {
        const double d0 = (double)b0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double c0 = (double)C[(size_t)i0 * 3 + k], c1 = (double)C[(size_t)i1 * 3 + k], c2 = (double)C[(size_t)i2 * 3 + k];
            const float v = (float)__dadd_rn(__dadd_rn(__dmul_rn(c0, d0), __dmul_rn(c1, d1)), __dmul_rn(c2, d2));
            out_col[(size_t)i * 3 + k] = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
        }
    }
    if (out_face) out_face[i] = f;
    if (out_bary) {
        out_bary[(size_t)i * 3 + 0] = b0;
        out_bary[(size_t)i * 3 + 1] = r1;
        out_bary[(size_t)i * 3 + 2] = r2;
    }
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
