// mesh_sample.h -- the device bodies of the surface sampler, stated once for mesh_sample.hip (one mesh per call) and
// mesh_sample_ragged.hip (c meshes per call): a face's area and its checks, the per-wave fold into a mesh's header, the
// weights and their scan inside a chunk of kMsChunk faces, the scan of a mesh's chunk sums with its status word, Philox, the
// two searches and the placement of a sample.  The definition is include/genpc_hip.h's (genpc_mesh_sample).  Every body
// sees ONE mesh through pointers its caller has already moved to that mesh: an index it forms is the mesh's own.
#pragma once
#include "common.h"

namespace genpc {

constexpr int kMsBlock = 256;
constexpr int kMsChunk = 1024;                    // faces per scan workgroup: kMsBlock lanes x 4
constexpr int kMsMaxFaces = 1 << 24;
constexpr int kMsScanBlock = 1024;                // the one workgroup that scans a mesh's chunk sums,
constexpr int kMsScanPerLane = 16;                // 16 a lane: kMsMaxFaces / kMsChunk = 16384 sums
constexpr int kMsStage = 2048;                    // chunk sums staged in LDS by the sampling kernel
typedef unsigned long long u64;

struct MsHeader {                                 // zeroed at the head of every call
    u64 amax_bits;                                // max_f A_f as its bit pattern
    int bad;                                      // a face with an index outside [0, nv) or a non-finite vertex
};

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

// A_f of face f (0 for a failing face).  The three indices are checked against [0, nv) BEFORE a vertex is loaded and the nine
// coordinates for finiteness; `bad` says that the face failed.
__device__ __forceinline__ double ms_face_area(int nv, const float *__restrict__ V, const int *__restrict__ F, int f, bool &bad)
{
    double a = 0.0;
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
    return a;
}

// the wave's maximum (areas are >= 0 and never NaN) and whether any of its faces failed, folded into the mesh's header: one
// integer atomic max on the bit pattern (positive doubles order as their bits) and one or per wave.  All 64 lanes active.
__device__ __forceinline__ void ms_wave_fold(double a, bool bad, MsHeader *__restrict__ hdr)
{
    double m = a;
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) m = fmax(m, __shfl_xor(m, d));
    const bool any_bad = __ballot(bad) != 0;
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (m > 0.0) atomicMax(&hdr->amax_bits, (u64)__double_as_longlong(m));
        if (any_bad) atomicOr(&hdr->bad, 1);
    }
}

// Chunk `chunk` of a mesh of nf faces, a workgroup of kMsBlock lanes, four consecutive faces a lane: weights, the inclusive
// scan INSIDE the chunk (written over the areas in cum) and the chunk's sum -> *chunk_slot.  s_w: kMsBlock / kWave words of LDS.
__device__ __forceinline__ void ms_weight_scan_chunk(int nf, u64 *__restrict__ cum, const MsHeader *__restrict__ hdr, int chunk,
                                                     u64 *__restrict__ chunk_slot, u64 *s_w)
{
    const u64 amax_bits = hdr->amax_bits;
    // Amax is 0 (every weight 0) or a normal double (>= 2^-596 for fp32 coordinates): ilogb is its exponent field
    const int shift = amax_bits ? 38 - ((int)(amax_bits >> 52) - 1023) : 0;
    const int base = chunk * kMsChunk + threadIdx.x * 4;
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
    if (threadIdx.x == kMsBlock - 1) *chunk_slot = before + w[3];
}

// One workgroup of kMsScanBlock lanes, 16 consecutive chunk sums a lane (nf <= 2^24: at most 16384 chunks), scans a mesh's
// sums in place and writes its status word.  s_w: kMsScanBlock / kWave words of LDS.
__device__ __forceinline__ void ms_chunk_scan(int chunks, u64 *__restrict__ chunk_sum, const MsHeader *__restrict__ hdr,
                                              int *__restrict__ out_status, u64 *s_w)
{
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

// Sample i of a mesh: Philox counter i, row i of the mesh's outputs.  Two searches: the chunk (first chunk whose inclusive sum
// exceeds t), then the face inside it against t minus the chunks before -- the same face as one search of the global
// cumulative weights, which are never materialised.  sums: the mesh's scanned chunk sums, in LDS or in global memory.
__device__ __forceinline__ void ms_draw(const float *__restrict__ V, const float *__restrict__ C, int nf, const int *__restrict__ F,
                                        const u64 *__restrict__ cum, const u64 *sums, int chunks, int i, uint32_t seed_lo,
                                        uint32_t seed_hi, float *__restrict__ out_xyz, float *__restrict__ out_col,
                                        int *__restrict__ out_face, float *__restrict__ out_bary)
{
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
    // cum[f] > tl >= cum[f - 1]: the face has a positive weight, so it passed ms_face_area's checks
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
