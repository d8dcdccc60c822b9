// depth_prompt_ragged.hip -- everything of DepthPrompting.getDepth after hidden-point removal, for S scans of different sizes in
// one call (genpc_depth_prompt_ragged), and ScaleAdapter.colorPoint for S scans (genpc_gather_colors_ragged).
//
// Per scan the definition is getDepth's: uv / depth through the chosen camera and its opposite with the bits of genpc_get_uvs
// on that scan alone (project_math.h's statements; with two cameras per scan every (camera, point) is divided exactly once --
// the approximate / exact split of project.hip pays off at 1024 cameras, not at two), the two sums of visible depths that pick
// one of the two rows, uvToPixels, and the three paints and two masks of getRawDepth.  A pixel's owner is the highest point
// index among the visible points that cover it: the rank inside the visible subset ascends with the index, so an integer
// atomicMax of the index elects the point pix[visible] elects -- no compaction, no order dependence.  The two paints at
// point_size (colours, grey level) share one owner plane; the paint at point_size * mask_pixel_rate has the other.
// The work numbering, the summation order, the launch count and the scratch are depth_prompt_ragged_plan.h's.
#include "common.h"
#include "project_math.h"
#include "depth_prompt_ragged_plan.h"
#include "../../include/genpc_hip.h"

namespace genpc {

static_assert(kDpMaxScans == GENPC_DEPTH_PROMPT_RAGGED_MAX_SCANS, "the header exports the bound");
static_assert(kDpBlock == 4 * kWave, "a chunk's partial is ((w0 + w1) + w2) + w3");

typedef float dp_f4u __attribute__((ext_vector_type(4), aligned(4)));

struct DepthPromptArgs {
    DepthPromptRaggedTable t;                  // (first: the layout of the kernel arguments)
    const float *xyz, *rgb, *cams;
    const unsigned char *vis;
    float focal, A, B, padmul;
    int rescale, res, ps1, ps2;
    unsigned *keys;                            // [c][kDpKeysPerScan]
    int *owner;                                // [c][2][res * res]
    double *part;                              // [items][2]
    float *rec;                                // [c][kDpRecFloats]
    float *uv, *depth;
    int *pix;
    unsigned char *visible;
    int *chosen;
    double *sums;
    float *images;
    int *status;
};
static_assert(sizeof(DepthPromptArgs) <= 4096, "the table must fit the kernel arguments");

// the thread's kDpPer points of the scan that starts at packed position o: i0 .. i0 + kDpPer - 1, those below n
__device__ __forceinline__ void dp_load_points(const float *__restrict__ xyz, int o, int i0, int n, float (&p)[kDpPer][3])
{
    const float *q = xyz + ((size_t)o + i0) * 3;
    if (i0 + kDpPer <= n) {
        const dp_f4u a = *(const dp_f4u *)q, b = *(const dp_f4u *)(q + 4), c = *(const dp_f4u *)(q + 8);
        p[0][0] = a.x; p[0][1] = a.y; p[0][2] = a.z; p[1][0] = a.w;
        p[1][1] = b.x; p[1][2] = b.y; p[2][0] = b.z; p[2][1] = b.w;
        p[2][2] = c.x; p[3][0] = c.y; p[3][1] = c.z; p[3][2] = c.w;
    } else {
#pragma unroll
        for (int u = 0; u < kDpPer; u++) {
            const bool in = i0 + u < n;
#pragma unroll
            for (int k = 0; k < 3; k++) p[u][k] = in ? q[u * 3 + k] : 0.0f;
        }
    }
}

__device__ __forceinline__ double dp_wave_sum(double x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, kWave);
    return x;
}
__device__ __forceinline__ unsigned dp_wave_min(unsigned x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = min(x, (unsigned)__shfl_xor((int)x, o, kWave));
    return x;
}

// box: both cameras' exact NDC boxes and visible depth ranges (integer atomic minima of order-preserving keys) and the chunk's
// two partial sums (steps 1-3 of the plan header's order)
__global__ __launch_bounds__(kDpBlock) void depth_prompt_box_kernel(DepthPromptArgs a)
{
    __shared__ unsigned s_keys[kDpBlock / kWave][kDpKeysPerScan];
    __shared__ double s_sum[kDpBlock / kWave][2];
    const int item = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int j = depth_prompt_scan_of(a.t, item), o = a.t.off[j], n = a.t.off[j + 1] - o;
    const int base = (item - depth_prompt_first_item(a.t.off, j)) << kDpChunkShift;
    if (base >= n) return;                             // (uniform: the one spare item of a scan, or an empty scan)
    const int i0 = base + tid * kDpPer;
    float p[kDpPer][3];
    dp_load_points(a.xyz, o, i0, n, p);
    unsigned key[kDpKeysPerScan];
#pragma unroll
    for (int k = 0; k < kDpKeysPerScan; k++) key[k] = 0xffffffffu;
    double sum[2] = {0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const float *V = a.cams + ((size_t)j * 2 + r) * 12;
        float v[12];
#pragma unroll
        for (int k = 0; k < 12; k++) v[k] = V[k];
        const unsigned char *vis = a.vis + 2 * (size_t)o + (size_t)r * n;
#pragma unroll
        for (int u = 0; u < kDpPer; u++) {
            if (i0 + u >= n) continue;
            float ox, oy, oz;
            project_point(v, a.focal, a.A, a.B, p[u][0], p[u][1], p[u][2], ox, oy, oz);
            const unsigned kx = f2key(ox), ky = f2key(oy);
            key[r * 4 + 0] = min(key[r * 4 + 0], kx); key[r * 4 + 1] = min(key[r * 4 + 1], ky);
            key[r * 4 + 2] = min(key[r * 4 + 2], ~kx); key[r * 4 + 3] = min(key[r * 4 + 3], ~ky);
            if (vis[i0 + u]) {
                const unsigned kz = f2key(oz);
                key[8 + r * 2 + 0] = min(key[8 + r * 2 + 0], kz); key[8 + r * 2 + 1] = min(key[8 + r * 2 + 1], ~kz);
                sum[r] += (double)oz;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kDpKeysPerScan; k++) key[k] = dp_wave_min(key[k]);
    sum[0] = dp_wave_sum(sum[0]);
    sum[1] = dp_wave_sum(sum[1]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kDpKeysPerScan; k++) s_keys[wave][k] = key[k];
        s_sum[wave][0] = sum[0]; s_sum[wave][1] = sum[1];
    }
    __syncthreads();
    if (tid < kDpKeysPerScan) {
        const unsigned m = min(min(s_keys[0][tid], s_keys[1][tid]), min(s_keys[2][tid], s_keys[3][tid]));
        if (m != 0xffffffffu) atomicMin(&a.keys[(size_t)j * kDpKeysPerScan + tid], m);
    }
    if (tid < 2) a.part[(size_t)item * 2 + tid] = ((s_sum[0][tid] + s_sum[1][tid]) + s_sum[2][tid]) + s_sum[3][tid];
}

// decide: one wave per scan -- steps 4-5 of the order, the choice, the status and the chosen camera's record
__global__ __launch_bounds__(kWave) void depth_prompt_decide_kernel(DepthPromptArgs a)
{
    const int j = blockIdx.x, lane = threadIdx.x;
    const int n = a.t.off[j + 1] - a.t.off[j];
    if (n == 0) {                                      // refused by its number; nothing else of the scan is written
        if (lane == 0) a.status[j] = -1;
        return;
    }
    const int chunks = depth_prompt_chunks(n), first = depth_prompt_first_item(a.t.off, j);
    double s0 = 0.0, s1 = 0.0;
    for (int k = lane; k < chunks; k += kWave) {
        s0 += a.part[(size_t)(first + k) * 2 + 0];
        s1 += a.part[(size_t)(first + k) * 2 + 1];
    }
    s0 = dp_wave_sum(s0);
    s1 = dp_wave_sum(s1);
    if (lane != 0) return;
    const int ch = s0 >= s1 ? 0 : 1;
    a.sums[(size_t)j * 2 + 0] = s0;
    a.sums[(size_t)j * 2 + 1] = s1;
    a.chosen[j] = ch;
    a.status[j] = 1;
    const unsigned *kq = a.keys + (size_t)j * kDpKeysPerScan;
    float *rec = a.rec + (size_t)j * kDpRecFloats;
    float cx, cy, sc;
    project_box_centre(key2f(kq[ch * 4 + 0]), key2f(kq[ch * 4 + 1]), key2f(~kq[ch * 4 + 2]), key2f(~kq[ch * 4 + 3]), cx, cy, sc);
    rec[0] = cx; rec[1] = cy; rec[2] = sc;
    rec[3] = key2f(kq[8 + ch * 2 + 0]);                // dmin, dmax over the chosen row's visible depths
    rec[4] = key2f(~kq[8 + ch * 2 + 1]);
}

// write: the chosen row's uv, depth, pixels and visibility; a visible point stamps its index into both owner planes
__global__ __launch_bounds__(kDpBlock) void depth_prompt_write_kernel(DepthPromptArgs a)
{
    const int item = blockIdx.x, tid = threadIdx.x;
    const int j = depth_prompt_scan_of(a.t, item), o = a.t.off[j], n = a.t.off[j + 1] - o;
    const int base = (item - depth_prompt_first_item(a.t.off, j)) << kDpChunkShift;
    if (base >= n) return;                             // (uniform)
    const int i0 = base + tid * kDpPer;
    if (i0 >= n) return;
    float p[kDpPer][3];
    dp_load_points(a.xyz, o, i0, n, p);
    const int ch = a.chosen[j], res = a.res;
    const float *rec = a.rec + (size_t)j * kDpRecFloats;
    const float cx = rec[0], cy = rec[1], sc = rec[2];
    const float *V = a.cams + ((size_t)j * 2 + ch) * 12;
    float v[12];
#pragma unroll
    for (int k = 0; k < 12; k++) v[k] = V[k];
    const unsigned char *vis = a.vis + 2 * (size_t)o + (size_t)ch * n;
    int *own1 = a.owner + (size_t)j * 2 * res * res, *own2 = own1 + (size_t)res * res;
#pragma unroll
    for (int u = 0; u < kDpPer; u++) {
        const int i = i0 + u;
        if (i >= n) break;
        float ox, oy, oz;
        project_point(v, a.focal, a.A, a.B, p[u][0], p[u][1], p[u][2], ox, oy, oz);
        const float uu = project_rescale(ox, cx, sc, a.padmul, a.rescale), vv = project_rescale(oy, cy, sc, a.padmul, a.rescale);
        const int pr = uv_pixel(vv, (float)res, res - 1), pc = uv_pixel(uu, (float)res, res - 1);      // (row, col): swapped
        const unsigned char vb = vis[i];
        const size_t q = (size_t)o + i;
        a.uv[q * 2 + 0] = uu; a.uv[q * 2 + 1] = vv;
        a.depth[q] = oz;
        a.pix[q * 2 + 0] = pr; a.pix[q * 2 + 1] = pc;
        a.visible[q] = vb ? 1 : 0;
        if (!vb) continue;
        // pr, pc lie in [0, res - 1]; the stamps are clipped to the image
        for (int s = 0; s < 2; s++) {
            const int ps = s ? a.ps2 : a.ps1;
            int *own = s ? own2 : own1;
            const int r0 = max(pr - (ps - 1), 0), r1 = min(pr + (ps - 1), res - 1);
            const int c0 = max(pc - (ps - 1), 0), c1 = min(pc + (ps - 1), res - 1);
            for (int rr = r0; rr <= r1; rr++)
                for (int cc = c0; cc <= c1; cc++) atomicMax(&own[(size_t)rr * res + cc], i);
        }
    }
}

// image: sparse_img, raw_depth, hole_mask1, hole_mask2 of every scan from its owner planes, vertically flipped (getRawDepth)
__global__ __launch_bounds__(kDpBlock) void depth_prompt_image_kernel(DepthPromptArgs a)
{
#pragma clang fp contract(off)
    const int j = blockIdx.y, res = a.res;
    const int o = a.t.off[j], n = a.t.off[j + 1] - o;
    const int t = blockIdx.x * kDpBlock + threadIdx.x;
    if (n == 0 || t >= res * res) return;
    const int r = t / res, c = t - r * res;
    const int *own1 = a.owner + (size_t)j * 2 * res * res, *own2 = own1 + (size_t)res * res;
    const int o1 = own1[t], o2 = own2[t];
    const float *rec = a.rec + (size_t)j * kDpRecFloats;
    float grey = 0.0f;
    if (o1 >= 0) {
        const float dmin = rec[3], dmax = rec[4], d = a.depth[(size_t)o + o1];
        grey = __fadd_rn(0.1f, __fmul_rn(0.8f, __fsub_rn(1.0f, __fsub_rn(d, dmin) / __fsub_rn(dmax, dmin))));
    }
    const size_t plane = (size_t)res * res, at = (size_t)(res - 1 - r) * res + c;
    float *img = a.images + (size_t)j * 12 * plane;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float c1 = o1 >= 0 ? a.rgb[((size_t)o + o1) * 3 + k] : 0.0f;
        const float c2 = o2 >= 0 ? a.rgb[((size_t)o + o2) * 3 + k] : 0.0f;
        // getRawDepth's masks, per channel: a colour channel that is exactly 0 counts as background in that channel
        const float all_front = c2 != 0.0f ? 1.0f : 0.0f, all_back = __fsub_rn(1.0f, all_front);
        const float back = __fsub_rn(1.0f, c1 != 0.0f ? 1.0f : 0.0f);
        const float h1 = (float)((int)__fmul_rn(all_back, 255.0f) ^ (int)__fmul_rn(back, 255.0f)) / 255.0f;
        const float h2 = (float)((int)__fmul_rn(all_front, 255.0f) ^ (int)__fmul_rn(back, 255.0f)) / 255.0f;
        img[(0 * 3 + k) * plane + at] = c1;
        img[(1 * 3 + k) * plane + at] = grey;
        img[(2 * 3 + k) * plane + at] = h1;
        img[(3 * 3 + k) * plane + at] = h2;
    }
}

// colorPoint for S scans: block = 256 consecutive points of one scan (ragged_offsets.h's item numbering, shift 8)
constexpr int kGcShift = 8;
static_assert(kDpBlock == 1 << kGcShift, "one thread per point of an item");
struct GatherRaggedArgs {
    DepthPromptRaggedTable t;
    const float *uv, *imgs;
    int ch, h, w, clip_max;
    float res;
    int *pix;
    float *out;
};
__global__ __launch_bounds__(kDpBlock) void gather_colors_ragged_kernel(GatherRaggedArgs a)
{
    const int item = blockIdx.x;
    const int j = ragged_item_owner(a.t.off, a.t.c, item, kGcShift), o = a.t.off[j], n = a.t.off[j + 1] - o;
    const int i = ((item - ((o >> kGcShift) + j)) << kGcShift) + threadIdx.x;
    if (i >= n) return;
    const size_t q = (size_t)o + i;
    const int r = uv_pixel(a.uv[q * 2 + 1], a.res, a.clip_max), c = uv_pixel(a.uv[q * 2 + 0], a.res, a.clip_max);
    if (a.pix) { a.pix[q * 2 + 0] = r; a.pix[q * 2 + 1] = c; }
    const float *img = a.imgs + (size_t)j * a.ch * a.h * a.w;
    for (int k = 0; k < a.ch; k++) a.out[q * a.ch + k] = img[((size_t)k * a.h + (a.h - 1 - r)) * a.w + c];
}

}  // namespace genpc

GENPC_API int genpc_depth_prompt_ragged(int c, const int *off, const float *xyz, const float *rgb, const float *cams,
                                        const unsigned char *vis, float focal, float znear, float zfar, int rescale, float padmul,
                                        int res, int point_size, int mask_pixel_rate, float *uv, float *depth, int *pix,
                                        unsigned char *visible, int *chosen, double *sums, float *images, int *status, void *stream)
{
    using namespace genpc;
    const char *fn = "genpc_depth_prompt_ragged";
    if (const char *what = depth_prompt_ragged_fault(c, off, res, point_size, mask_pixel_rate)) return ragged_refuse(fn, what);
    if (c == 0) return 1;
    if (!cams || !chosen || !sums || !images || !status) return ragged_refuse(fn, "null pointer");
    if (off[c] > 0 && (!xyz || !rgb || !vis || !uv || !depth || !pix || !visible)) return ragged_refuse(fn, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    const DepthPromptRaggedPlan plan = depth_prompt_ragged_plan(c, off, res);
    DepthPromptArgs a{};
    unsigned *fill;
    WsLayout L;
    L.add(fill, (size_t)plan.fill_ints);
    L.add(a.part, (size_t)plan.items * 2);
    L.add(a.rec, (size_t)c * kDpRecFloats);
    if (!ws_alloc(L, kWsDepthPromptRagged, st)) return 0;
    a.keys = fill;
    a.owner = (int *)(fill + (size_t)c * kDpKeysPerScan);
    a.t.c = c;
    ragged_pad_copy(a.t.off, off, c);
    a.xyz = xyz; a.rgb = rgb; a.cams = cams; a.vis = vis;
    a.focal = focal; a.padmul = padmul;
    project_depth_constants(znear, zfar, a.A, a.B);
    a.rescale = rescale ? 1 : 0; a.res = res; a.ps1 = point_size; a.ps2 = point_size * mask_pixel_rate;
    a.uv = uv; a.depth = depth; a.pix = pix; a.visible = visible;
    a.chosen = chosen; a.sums = sums; a.images = images; a.status = status;
    if (!check(hipMemsetAsync(fill, 0xff, (size_t)plan.fill_ints * 4, st), "depth_prompt_ragged: memset of the keys and owner planes")) return 0;
    hipLaunchKernelGGL(depth_prompt_box_kernel, dim3(plan.items), dim3(kDpBlock), 0, st, a);
    hipLaunchKernelGGL(depth_prompt_decide_kernel, dim3(c), dim3(kWave), 0, st, a);
    hipLaunchKernelGGL(depth_prompt_write_kernel, dim3(plan.items), dim3(kDpBlock), 0, st, a);
    hipLaunchKernelGGL(depth_prompt_image_kernel, dim3(ceil_div(res * res, kDpBlock), c), dim3(kDpBlock), 0, st, a);
    return check(hipGetLastError(), "depth_prompt_ragged launch") ? 1 : 0;
}

GENPC_API int genpc_depth_prompt_ragged_plan(int c, const int *off, int res, int point_size, int mask_pixel_rate, long long out[7])
{
    using namespace genpc;
    const char *fn = "genpc_depth_prompt_ragged_plan";
    if (!out) return ragged_refuse(fn, "null pointer");
    for (int k = 0; k < 7; k++) out[k] = 0;
    out[4] = -1;
    if (const char *what = depth_prompt_ragged_fault(c, off, res, point_size, mask_pixel_rate)) return ragged_refuse(fn, what);
    const DepthPromptRaggedPlan p = depth_prompt_ragged_plan(c, off, res);
    out[0] = p.items; out[1] = p.launches; out[2] = p.memsets; out[3] = p.refused; out[4] = p.first_refused;
    out[5] = p.fill_ints; out[6] = p.ws_bytes;
    return 1;
}

GENPC_API int genpc_gather_colors_ragged(int c, const int *off, const float *uv, const float *imgs, int ch, int h, int w, float res,
                                         int clip_max, int *pix, float *out, void *stream)
{
    using namespace genpc;
    const char *fn = "genpc_gather_colors_ragged";
    if (c < 0) return ragged_refuse(fn, "negative number of scans");
    if (c > kDpMaxScans) return ragged_refuse(fn, "more than 256 scans in one call");
    if (c == 0) return 1;
    if (!off) return ragged_refuse(fn, "null offset table");
    if (const char *e = ragged_offsets_fault(c, off)) return ragged_refuse(fn, e);
    if (off[c] > kDpMaxPoints) return ragged_refuse(fn, "more than 2^28 points");
    if (ch < 1 || h < 1 || w < 1 || clip_max < 0 || clip_max >= h || clip_max >= w) return ragged_refuse(fn, "the pixel grid exceeds the images");
    if (off[c] == 0) return 1;
    if (!uv || !imgs || !out) return ragged_refuse(fn, "null pointer");
    GatherRaggedArgs a{};
    a.t.c = c;
    ragged_pad_copy(a.t.off, off, c);
    a.uv = uv; a.imgs = imgs; a.ch = ch; a.h = h; a.w = w; a.clip_max = clip_max; a.res = res; a.pix = pix; a.out = out;
    hipLaunchKernelGGL(gather_colors_ragged_kernel, dim3((off[c] >> kGcShift) + c), dim3(kDpBlock), 0, (hipStream_t)stream, a);
    return check(hipGetLastError(), "gather_colors_ragged launch") ? 1 : 0;
}
