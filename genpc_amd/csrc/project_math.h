// project_math.h -- the projection arithmetic of DepthPrompting.getUvs / uvToPixels, stated once for project.hip (any number of
// cameras, one cloud) and depth_prompt_ragged.hip (two cameras per scan, many scans): the order-preserving keys of the exact
// bounding box, the pinhole projection of one point, the box's centre and extent, the rescale of one NDC coordinate and the
// pixel of one uv coordinate.  Every operation is rounded on its own, in the order of oracle/genpc_oracle_geom.c.
// Device code: include after common.h.
#pragma once

namespace genpc {

// float -> unsigned key with the same ordering
__device__ __forceinline__ unsigned f2key(float f)
{
    unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k)
{
    // branch-free: the select form crashes hipcc 7.2's instruction selection inside project_write_kernel
    return __uint_as_float(k ^ ((unsigned)((int)~k >> 31) | 0x80000000u));
}

__device__ __forceinline__ void project_point(const float *v, float focal, float A, float B, float px, float py,
                                              float pz, float &ox, float &oy, float &oz)
{
    const float xc = __fadd_rn(__fmaf_rn(v[2], pz, __fmaf_rn(v[1], py, __fmul_rn(v[0], px))), v[3]);
    const float yc = __fadd_rn(__fmaf_rn(v[6], pz, __fmaf_rn(v[5], py, __fmul_rn(v[4], px))), v[7]);
    const float zc = __fadd_rn(__fmaf_rn(v[10], pz, __fmaf_rn(v[9], py, __fmul_rn(v[8], px))), v[11]);
    const float w = -zc;
    ox = __fmul_rn(focal, xc) / w;
    oy = __fmul_rn(focal, yc) / w;
    oz = __fmaf_rn(A, zc, B) / w;
}

// the NDC depth's two constants (kaolin's pinhole projection)
__host__ __device__ __forceinline__ void project_depth_constants(float znear, float zfar, float &A, float &B)
{
    A = (zfar + znear) / (znear - zfar);
    B = (2.0f * zfar * znear) / (znear - zfar);
}

// a camera's box -> centre and extent, DepthPrompting.py:246-262
__device__ __forceinline__ void project_box_centre(float mnx, float mny, float mxx, float mxy, float &cx, float &cy, float &sc)
{
    cx = __fmul_rn(__fadd_rn(mnx, mxx), 0.5f);       // == / 2.0f (exact scaling; a subnormal sum halves with the same rounding)
    cy = __fmul_rn(__fadd_rn(mny, mxy), 0.5f);
    const float sx = __fsub_rn(mxx, mnx), sy = __fsub_rn(mxy, mny);
    sc = sx > sy ? sx : sy;
}

// one NDC coordinate -> uv, DepthPrompting.py:263-268: about the box centre c with extent sc, or the whole NDC square
__device__ __forceinline__ float project_rescale(float o, float c, float sc, float padmul, int rescale)
{
    return rescale ? __fadd_rn(__fmul_rn(__fsub_rn(o, c) / sc, padmul), 0.5f) : __fmul_rn(__fadd_rn(o, 1.0f), 0.5f);
}

// DepthPrompting.py:179-184, ScaleAdapter.py:59-62: (uv * res).long(), clipped to [0, clip_max]
__device__ __forceinline__ int uv_pixel(float u, float res, int clip_max)
{
    const long long p = (long long)__fmul_rn(u, res);
    return (int)(p < 0 ? 0 : (p > clip_max ? clip_max : p));
}

}  // namespace genpc
