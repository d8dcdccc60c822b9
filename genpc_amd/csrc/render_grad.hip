// render_grad.hip -- the renderer of mask_render.hip as a differentiable operation of its own: b clouds drawn in one call with the
// blend the CALLER names (genpc_render_points), and the backward of those images for a caller's d L / d I, per point
// (genpc_render_points_backward): d L / d xyz and d L / d colour of every point.  The silhouette loss's own backward
// (mask_loss.hip mask_grad_kernel) chains the same gather straight into 13 pose sums; here the chain stops at the point.
//   render_image_kernel         the five planes of b images as [b, S, S, 3] (load_pixel: mask_image_kernel's bits)
//   render_w_kernel             per pixel, from the planes and G = d L / d I (tests/mask_loss_ref.py weights(), mask_weight 1):
//                                 blend 1:  W1 = m,        W4 = (G, G . I) / D'
//                                 blend 0:  W1 = T (G . A),  W4 = (O / D) (G, G . A),   1 / D := 0 where D = 0
//   render_grad_points_kernel   per point: the pixel centres of the disc's box exactly as mask_grad_kernel walks them -- eight lanes
//                               a point, lane s the rows r0 + s, r0 + s + 8, ..., columns ascending, rows with an empty chord
//                               skipped, the eight partial sums joined by that kernel's DPP tree, the same __expf and hardware
//                               reciprocal -- so the order of every sum is a function of the point and the image alone: no atomics,
//                               no workgroup waits for another, the same bits in every run, batch and stream.
//                                 grad_pts = (gu f4 iz, -gv f4 iz, -gzv)      (mask_grad_kernel's g[3]; doubles, stored as float)
//                                 grad_col[ch] = sum over the pixels with a > 0 of  W4.ch min(a, 0.999) exp(ze - W1)   (blend 1)
//                                                                                 W4.ch min(a, 0.999)                 (blend 0)
//                               The clamped pixels (a >= 0.999) count for the colour and for gz, not for gu, gv, grho.
//                               A point the camera does not see, or one with a coordinate (or a projection) that is not finite,
//                               gets +0 rows: decided at the head, before any index is formed.
// The loop body is restated here rather than shared with mask_grad_kernel: that kernel's code does not move.
// The ragged form (genpc_render_points_ragged, genpc_render_points_ragged_backward; its shape: render_ragged_plan.h): s clouds of
// different sizes, each with a radius of its own, packed by an element table.
//   render_ragged_tables_kernel    the element table and the radii travel BY VALUE in this launch's arguments (pose_ragged.hip's way)
//                                  and are written to scratch, where the other kernels read them with scalar loads
//   render_project_ragged_kernel   mask_project_kernel's unposed loop through the same device functions, the element's span from
//                                  the table and the element's own radius: uvr, zex (blend 1) and the tile lists.  The splat is
//                                  launch_mask_splat's, given the table, and the images are render_image_kernel's
//   render_grad_points_ragged_kernel   the gather's body with the element's span and radius
// Element j's bits are those of the equal-size entry points on element j alone with radius[j].
#include "mask.h"
#include "render_ragged_plan.h"
#include "../../include/genpc_hip.h"

namespace genpc {

// grid (blocks, b)
__global__ __launch_bounds__(kQBlock) void render_image_kernel(int P, const float *__restrict__ planes, float *__restrict__ img, int mode)
{
    const int e = blockIdx.y;
    planes += (size_t)e * 5 * P;
    img += (size_t)e * 3 * P;
    for (int q = blockIdx.x * kQBlock + threadIdx.x; q < P; q += gridDim.x * kQBlock) {
        const PxImg px = load_pixel(planes, P, q, mode);
        img[(size_t)q * 3 + 0] = px.I[0];
        img[(size_t)q * 3 + 1] = px.I[1];
        img[(size_t)q * 3 + 2] = px.I[2];
    }
}

// grid (blocks, b); mode: 2 blend 1, 0 blend 0
__global__ __launch_bounds__(kQBlock) void render_w_kernel(int P, const float *__restrict__ planes, int mode,
                                                           const float *__restrict__ grad_img, float *__restrict__ W1,
                                                           float4 *__restrict__ W4)
{
    const int e = blockIdx.y;
    planes += (size_t)e * 5 * P;
    grad_img += (size_t)e * 3 * P;
    W1 += (size_t)e * P;
    W4 += (size_t)e * P;
    for (int q = blockIdx.x * kQBlock + threadIdx.x; q < P; q += gridDim.x * kQBlock) {
        const PxImg im = load_pixel(planes, P, q, mode);
        const float G[3] = {grad_img[(size_t)q * 3 + 0], grad_img[(size_t)q * 3 + 1], grad_img[(size_t)q * 3 + 2]};
        if (mode == 2) {
            const float sI = G[0] * im.I[0] + G[1] * im.I[1] + G[2] * im.I[2];
            W1[q] = im.T;
            W4[q] = make_float4(im.iD * G[0], im.iD * G[1], im.iD * G[2], im.iD * sI);
        } else {
            const float sA = G[0] * im.A[0] + G[1] * im.A[1] + G[2] * im.A[2];
            const float od = im.O * im.iD;
            W1[q] = im.T * sA;
            W4[q] = make_float4(od * G[0], od * G[1], od * G[2], od * sA);
        }
    }
}

constexpr int kRenderSub = 8;      // lanes a point
static_assert(kRenderSub == kRenderRaggedSub, "render_ragged_plan.h sizes the ragged gather's grid with it");

// the eight lanes of a point: quads by permutation, then the mirror image within the eight (mask_grad_kernel's tree)
__device__ __forceinline__ float sum8(float x)
{
    x += dpp_or_zero<0xB1>(x);
    x += dpp_or_zero<0x4E>(x);
    x += dpp_or_zero<0x141>(x);
    return x;
}

// The gather of one element's points, stated once for the equal-size and the ragged kernel below: the n points at pts (col, grad_pts,
// grad_col alike) against the element's planes W1, W4 [S * S]; bx of gx: this block among the element's.  COL: grad_col is written.
template <int BLEND, int COL>
__device__ __forceinline__ void render_grad_points_body(int n, const float *__restrict__ pts, const float *__restrict__ col, float radius,
                                                        int S, const float *__restrict__ W1, const float4 *__restrict__ W4,
                                                        float *__restrict__ grad_pts, float *__restrict__ grad_col, int bx, int gx)
{
    const float hs = 0.5f * S;
    const int sub = threadIdx.x & (kRenderSub - 1);
    const int per_block = kQBlock / kRenderSub;
    for (int j0 = bx * per_block; j0 < n; j0 += gx * per_block) {      // (block-uniform: every lane reaches the DPP sums)
        const int j = j0 + threadIdx.x / kRenderSub;
        const bool live = j < n;
        const int jj = live ? j : n - 1;
        const float vx = pts[(size_t)jj * 3 + 0], vy = pts[(size_t)jj * 3 + 1], vz = pts[(size_t)jj * 3 + 2];
        float cr = 1.0f, cg = 1.0f, cb = 1.0f;
        if (col) { cr = col[(size_t)jj * 3 + 0]; cg = col[(size_t)jj * 3 + 1]; cb = col[(size_t)jj * 3 + 2]; }
        // a coordinate that is not finite: the point is the origin from here on and its row +0
        const bool finite = isfinite(vx) && isfinite(vy) && isfinite(vz);
        const float p[3] = {finite ? vx : 0.0f, finite ? vy : 0.0f, finite ? vz : 0.0f};
        const SplatPt q = splat_project(p, radius, hs);
        const bool ok = live && finite && q.ok && isfinite(q.u) && isfinite(q.v) && isfinite(q.rho) && q.rho > 0.0f;
        float gu = 0.0f, gv = 0.0f, gr = 0.0f, gz = 0.0f, kr = 0.0f, kg = 0.0f, kb = 0.0f;
        const float ir2 = 1.0f / (q.rho * q.rho);
        const float ze = pulsar_ze(q.zv);
        if (ok) {
            const int c0 = max((int)floorf(q.u - q.rho - 0.5f), 0), c1 = min((int)ceilf(q.u + q.rho - 0.5f), S - 1);
            const int r0 = max((int)floorf(q.v - q.rho - 0.5f), 0), r1 = min((int)ceilf(q.v + q.rho - 0.5f), S - 1);
            const float rho2 = q.rho * q.rho;
            for (int r = r0 + sub; r <= r1; r += kRenderSub) {
                const float dy = (float)r + 0.5f - q.v;
                const float h2 = rho2 - dy * dy;
                if (h2 < -1e-5f * rho2) continue;
                const float h = sqrtf(fmaxf(h2, 0.0f));
                const int ca = max((int)floorf(q.u - h - 0.5f), c0), cz = min((int)ceilf(q.u + h - 0.5f), c1);
                for (int cc = ca; cc <= cz; cc++) {
                    const float dx = (float)cc + 0.5f - q.u;
                    const float d2 = dx * dx + dy * dy;
                    const float av = 1.0f - d2 * ir2;
                    if (av <= 0.0f) continue;
                    const float4 w4 = W4[(size_t)r * S + cc];
                    const float w1 = W1[(size_t)r * S + cc];
                    const float ac = fminf(av, kMaskAmax);
                    if (BLEND) {
                        const float ex = __expf(ze - w1);
                        if (COL) {
                            const float ae = ac * ex;
                            kr += w4.x * ae; kg += w4.y * ae; kb += w4.z * ae;
                        }
                        const float w = ((cr * w4.x + cg * w4.y) + (cb * w4.z - w4.w)) * ex;
                        gz += w * ac;
                        if (av >= kMaskAmax) continue;
                        gu += w * dx;
                        gv += w * dy;
                        gr += w * d2;
                        continue;
                    }
                    if (COL) { kr += w4.x * ac; kg += w4.y * ac; kb += w4.z * ac; }
                    if (av >= kMaskAmax) continue;      // clamped: no gradient to the position
                    const float w = w1 * __builtin_amdgcn_rcpf(1.0f - av) + ((cr * w4.x + cg * w4.y) + (cb * w4.z - w4.w));
                    gu += w * dx;
                    gv += w * dy;
                    gr += w * d2;
                }
            }
        }
        gu = sum8(gu); gv = sum8(gv); gr = sum8(gr);
        if (BLEND) gz = sum8(gz);
        if (COL) { kr = sum8(kr); kg = sum8(kg); kb = sum8(kb); }
        if (!live || sub != 0) continue;
        float o[3] = {0.0f, 0.0f, 0.0f};
        if (ok) {
            gu *= 2.0f * ir2; gv *= 2.0f * ir2; gr *= 2.0f * ir2 / q.rho;
            const double iz = 1.0 / (double)q.zv;
            const double f4 = (double)hs * kMaskFocal;
            const double gzv = (double)gu * (-f4 * p[0] * iz * iz) + (double)gv * (f4 * p[1] * iz * iz) + (double)gr * (-(double)q.rho * iz) +
                               (BLEND ? -(double)gz * (double)kPulsarZeK : 0.0);
            // (+ 0: a sum of no terms leaves -0 behind the signs above; a point without a gradient has +0 rows)
            o[0] = (float)((double)gu * f4 * iz) + 0.0f;
            o[1] = (float)(-(double)gv * f4 * iz) + 0.0f;
            o[2] = (float)(-gzv) + 0.0f;
        } else {
            kr = kg = kb = 0.0f;
        }
        grad_pts[(size_t)j * 3 + 0] = o[0];
        grad_pts[(size_t)j * 3 + 1] = o[1];
        grad_pts[(size_t)j * 3 + 2] = o[2];
        if (COL) {
            grad_col[(size_t)j * 3 + 0] = kr + 0.0f;
            grad_col[(size_t)j * 3 + 1] = kg + 0.0f;
            grad_col[(size_t)j * 3 + 2] = kb + 0.0f;
        }
    }
}

// 1-D grid of gx * nb blocks (xcd_block: an image's blocks gather its W planes -- 800 KB of W4 at 224 x 224 -- through one XCD's L2).
// pts, col (or null: white), grad_pts, grad_col [nb, n, 3]; W1, W4 [nb, S * S].  COL: grad_col is written.
template <int BLEND, int COL>
__global__ __launch_bounds__(kQBlock) void render_grad_points_kernel(int n, const float *__restrict__ pts, const float *__restrict__ col,
                                                                     float radius, int S, const float *__restrict__ W1,
                                                                     const float4 *__restrict__ W4, float *__restrict__ grad_pts,
                                                                     float *__restrict__ grad_col, int gx, int nb)
{
    const XcdBlock xb = xcd_block(gx, nb);
    const int e = xb.e;
    if (e >= nb) return;
    pts += (size_t)e * n * 3;
    if (col) col += (size_t)e * n * 3;
    grad_pts += (size_t)e * n * 3;
    if (COL) grad_col += (size_t)e * n * 3;
    W1 += (size_t)e * S * S;
    W4 += (size_t)e * S * S;
    render_grad_points_body<BLEND, COL>(n, pts, col, radius, S, W1, W4, grad_pts, grad_col, xb.x, gx);
}

// The ragged form: the same grid for the LARGEST element's gx; element e's span comes from the table on the device (pose_span), its
// radius from radius[e]; pts, col, grad_pts, grad_col are packed by the table, W1 and W4 stay per element.  A block that lies wholly
// beyond a short element leaves whole (the body's loop is block-uniform).
template <int BLEND, int COL>
__global__ __launch_bounds__(kQBlock) void render_grad_points_ragged_kernel(int nmax, const float *__restrict__ pts,
                                                                            const float *__restrict__ col, const float *__restrict__ radius,
                                                                            int S, const float *__restrict__ W1, const float4 *__restrict__ W4,
                                                                            float *__restrict__ grad_pts, float *__restrict__ grad_col, int gx,
                                                                            int nb, const int *__restrict__ off)
{
    const XcdBlock xb = xcd_block(gx, nb);
    const int e = xb.e;
    if (e >= nb) return;
    const PoseSpan sp = pose_span(off, e, nmax);
    if (xb.x * (kQBlock / kRenderSub) >= sp.n) return;
    pts += sp.base * 3;
    if (col) col += sp.base * 3;
    grad_pts += sp.base * 3;
    if (COL) grad_col += sp.base * 3;
    W1 += (size_t)e * S * S;
    W4 += (size_t)e * S * S;
    render_grad_points_body<BLEND, COL>(sp.n, pts, col, radius[e], S, W1, W4, grad_pts, grad_col, xb.x, gx);
}

struct RenderRaggedTablesArgs {
    int off[kRenderRaggedMax + 1];          // padded with off[s] (ragged_pad_copy)
    float radius[kRenderRaggedMax];
    int *doff;                              // [s + 1]
    float *dradius;                         // [s]
};
static_assert(sizeof(RenderRaggedTablesArgs) <= 4096, "the tables must fit the kernel arguments");

__global__ __launch_bounds__(kQBlock) void render_ragged_tables_kernel(RenderRaggedTablesArgs a, int s)
{
    const int i = blockIdx.x * kQBlock + threadIdx.x;
    if (i > s) return;
    a.doff[i] = a.off[i];
    if (i < s) a.dradius[i] = a.radius[i];
}

static int render_ragged_tables(int s, const int *off, const float *radius, int *doff, float *dradius, hipStream_t st)
{
    RenderRaggedTablesArgs a{};
    ragged_pad_copy(a.off, off, s);
    for (int j = 0; j < s; j++) a.radius[j] = radius[j];
    a.doff = doff; a.dradius = dradius;
    hipLaunchKernelGGL(render_ragged_tables_kernel, dim3(ceil_div(s + 1, kQBlock)), dim3(kQBlock), 0, st, a, s);
    return check(hipGetLastError(), "render_ragged_tables_kernel launch") ? 1 : 0;
}

// grid (blocks for the largest element, s): mask_project_kernel's unposed loop, element e's span from the table and its own radius.
// uvr[off[e] + j] = (u, v, rho, 1 / rho^2), rho = -1 for points the camera does not see; zex (blend 1): the depth exponents; bins: the
// per-tile index lists of element e (mask.h kTileCap), entries counted from the element's first point as the splat reads them.
__global__ __launch_bounds__(kQBlock) void render_project_ragged_kernel(int nmax, const float *__restrict__ v, const float *__restrict__ radius,
                                                                        int S, float4 *__restrict__ uvr, int *__restrict__ bins,
                                                                        float *__restrict__ zex, const int *__restrict__ off)
{
    const int e = blockIdx.y;
    const PoseSpan sp = pose_span(off, e, nmax);
    const int n = sp.n;                  // (block-uniform: bin_points_block has barriers)
    const float rad = radius[e];
    v += sp.base * 3;
    uvr += sp.base;
    if (zex) zex += sp.base;
    int *bin_cnt = bins ? bins + (size_t)e * bins_tiles(S) : nullptr;
    int *bin_idx = bins ? bins + (size_t)gridDim.y * bins_tiles(S) + (size_t)e * bins_tiles(S) * kTileCap : nullptr;
    const float hs = 0.5f * S;
    __shared__ int s_cnt[kBinTiles], s_base[kBinTiles];
    for (int j0 = blockIdx.x * kQBlock; j0 < n; j0 += gridDim.x * kQBlock) {
        const int j = j0 + threadIdx.x;
        const bool valid = j < n;
        const int jj = valid ? j : n - 1;
        const float p[3] = {v[(size_t)jj * 3 + 0], v[(size_t)jj * 3 + 1], v[(size_t)jj * 3 + 2]};
        const SplatPt q = splat_project(p, rad, hs);
        if (valid) uvr[j] = make_float4(q.u, q.v, q.ok ? q.rho : -1.0f, q.ok ? 1.0f / (q.rho * q.rho) : 0.0f);
        if (valid && zex) zex[j] = pulsar_ze(q.zv);
        if (bin_cnt) bin_points_block(bin_cnt, bin_idx, s_cnt, s_base, S, valid && q.ok, j, q.u, q.v, q.rho);
    }
}

static int render_refuse(const char *fn, const char *what)
{
    char msg[192];
    snprintf(msg, sizeof msg, "%s: %s", fn, what);
    set_error(msg);
    return -1;
}

// what both entry points refuse alike (null: the arguments stand)
static const char *render_args_bad(int b, int n, float radius, int size, int blend)
{
    if (b <= 0) return "b must be positive";
    if (n < 0) return "n must not be negative";
    if (size <= 0 || size > 8192) return "size must be in 1 .. 8192";
    if (!(radius > 0.0f)) return "radius must be positive";
    if (blend != 0 && blend != 1) return "blend must be 0 or 1";
    if ((long long)b * n > (1ll << 28) || (long long)b * size * size > (1ll << 28)) return "b * n and b * size * size must not exceed 2^28";
    return nullptr;
}

// the calling thread's render mode is `blend` while this object lives (launch_mask_splat reads the thread's mode)
struct RenderBlendScope {
    int prev;
    explicit RenderBlendScope(int blend) : prev(t_render_blend) { t_render_blend = blend; }
    ~RenderBlendScope() { t_render_blend = prev; }
};

}  // namespace genpc

GENPC_API int genpc_render_points(int b, int n, const float *pts, const float *col, float radius, int size, int blend, float *img,
                                  float *planes_out, void *stream)
{
    using namespace genpc;
    const char *fn = "genpc_render_points";
    if (const char *bad = render_args_bad(b, n, radius, size, blend)) return render_refuse(fn, bad);
    if (!img) return render_refuse(fn, "img is null");
    if (n > 0 && !pts) return render_refuse(fn, "pts is null");
    hipStream_t st = (hipStream_t)stream;
    const size_t P = (size_t)size * size;
    MaskScratch m;
    WsLayout L;
    m.layout(L, b, P, n > 0 ? n : 1);
    if (!ws_alloc(L, kWsRenderPoints, st)) return 0;
    if (!m.zero_bins(st)) return 0;
    {
        RenderBlendScope scope(blend);
        launch_mask_splat(b, n, pts, col, true, nullptr, 0, nullptr, 0, 0, radius, size, m, nullptr, st);
    }
    hipLaunchKernelGGL(render_image_kernel, dim3(lin_grid((long long)P), b), dim3(kQBlock), 0, st, (int)P, (const float *)m.planes, img,
                       blend ? 2 : 0);
    if (!check(hipGetLastError(), "render_points launch")) return 0;
    if (planes_out &&
        !check(hipMemcpyAsync(planes_out, m.planes, (size_t)b * 5 * P * sizeof(float), hipMemcpyDeviceToDevice, st), "hipMemcpyAsync(planes_out)"))
        return 0;
    return 1;
}

GENPC_API int genpc_render_points_backward(int b, int n, const float *pts, const float *col, float radius, int size, int blend,
                                           const float *planes, const float *grad_img, float *grad_pts, float *grad_col, void *stream)
{
    using namespace genpc;
    const char *fn = "genpc_render_points_backward";
    if (const char *bad = render_args_bad(b, n, radius, size, blend)) return render_refuse(fn, bad);
    if (n == 0) return 1;
    if (!pts) return render_refuse(fn, "pts is null");
    if (!planes) return render_refuse(fn, "planes is null");
    if (!grad_img) return render_refuse(fn, "grad_img is null");
    if (!grad_pts) return render_refuse(fn, "grad_pts is null");
    hipStream_t st = (hipStream_t)stream;
    const size_t P = (size_t)size * size;
    float *W1;
    float4 *W4;
    WsLayout L;
    L.add(W1, (size_t)b * P);
    L.add(W4, (size_t)b * P);
    if (!ws_alloc(L, kWsRenderPointsGrad, st)) return 0;
    hipLaunchKernelGGL(render_w_kernel, dim3(lin_grid((long long)P), b), dim3(kQBlock), 0, st, (int)P, planes, blend ? 2 : 0, grad_img, W1, W4);
    const int gx = lin_grid((long long)n * kRenderSub);
#define GENPC_LAUNCH_RENDER_GRAD(BL, CO)                                                                                              \
    hipLaunchKernelGGL((render_grad_points_kernel<BL, CO>), dim3(gx * b), dim3(kQBlock), 0, st, n, pts, col, radius, size, (const float *)W1, \
                       (const float4 *)W4, grad_pts, grad_col, gx, b)
    if (blend) { if (grad_col) GENPC_LAUNCH_RENDER_GRAD(1, 1); else GENPC_LAUNCH_RENDER_GRAD(1, 0); }
    else { if (grad_col) GENPC_LAUNCH_RENDER_GRAD(0, 1); else GENPC_LAUNCH_RENDER_GRAD(0, 0); }
#undef GENPC_LAUNCH_RENDER_GRAD
    return check(hipGetLastError(), "render_points_backward launch") ? 1 : 0;
}

// a refused ragged call: "<fn>: <why>" recorded, -1 returned (the radius names its element)
static int render_ragged_refuse(const char *fn, const genpc::RenderRaggedPlan &plan)
{
    char why[128];
    genpc::render_ragged_refusal(plan, why, sizeof why);
    return genpc::ragged_refuse(fn, why);
}

GENPC_API int genpc_render_ragged_plan(int s, const int *off, const float *radius, int size, int blend, int out[12])
{
    using namespace genpc;
    const char *fn = "genpc_render_ragged_plan";
    if (!out) return ragged_refuse(fn, "null output");
    for (int k = 0; k < 12; k++) out[k] = 0;
    out[0] = kRenderRaggedMax;
    RenderRaggedAsk ask;
    ask.s = s; ask.off = off; ask.radius = radius; ask.size = size; ask.blend = blend;
    const RenderRaggedPlan plan = render_ragged_plan(ask);
    if (plan.refuse) { out[1] = plan.refuse_element; return render_ragged_refuse(fn, plan); }
    const long long cap = 0x7fffffffll;
    out[1] = -1; out[2] = plan.s; out[3] = plan.nmax; out[4] = (int)std::min(plan.total, cap); out[5] = plan.pixels; out[6] = plan.g_proj;
    out[7] = plan.g_pix; out[8] = plan.gx; out[9] = (int)std::min(plan.grad_blocks, cap); out[10] = (int)std::min((long long)plan.nmax_piece, cap);
    out[11] = (int)std::min((long long)plan.w_pixels, cap);
    return 1;
}

GENPC_API int genpc_render_points_ragged(int s, const int *off, const float *pts, const float *col, const float *radius, int size, int blend,
                                         float *img, float *planes_out, void *stream)
{
    using namespace genpc;
    const char *fn = "genpc_render_points_ragged";
    RenderRaggedAsk ask;
    ask.s = s; ask.off = off; ask.radius = radius; ask.size = size; ask.blend = blend;
    ask.pts = pts != nullptr; ask.img = img != nullptr;
    const RenderRaggedPlan plan = render_ragged_plan(ask);
    if (plan.refuse) return render_ragged_refuse(fn, plan);
    hipStream_t st = (hipStream_t)stream;
    const size_t P = (size_t)plan.pixels;
    MaskScratch m;
    int *doff;
    float *dradius;
    WsLayout L;
    L.add(doff, plan.table_ints);
    L.add(dradius, plan.table_floats);
    m.layout(L, plan.s, P, plan.nmax_piece);
    if (!ws_alloc(L, kWsRenderPointsRagged, st)) return 0;
    if (!m.zero_bins(st)) return 0;
    if (!render_ragged_tables(plan.s, off, radius, doff, dradius, st)) return 0;
    hipLaunchKernelGGL(render_project_ragged_kernel, dim3(plan.g_proj, plan.s), dim3(kQBlock), 0, st, plan.nmax, pts, (const float *)dradius, size,
                       m.uvr, use_bins(size) ? m.bins : (int *)nullptr, blend ? m.zex : (float *)nullptr, (const int *)doff);
    {
        RenderBlendScope scope(blend);
        launch_mask_splat(plan.s, plan.nmax, pts, col, /*project*/ false, nullptr, 0, nullptr, 0, 0, 0.0f, size, m, nullptr, st, doff);
    }
    hipLaunchKernelGGL(render_image_kernel, dim3(plan.g_pix, plan.s), dim3(kQBlock), 0, st, (int)P, (const float *)m.planes, img, blend ? 2 : 0);
    if (!check(hipGetLastError(), "render_points_ragged launch")) return 0;
    if (planes_out &&
        !check(hipMemcpyAsync(planes_out, m.planes, (size_t)plan.s * 5 * P * sizeof(float), hipMemcpyDeviceToDevice, st), "hipMemcpyAsync(planes_out)"))
        return 0;
    return 1;
}

GENPC_API int genpc_render_points_ragged_backward(int s, const int *off, const float *pts, const float *col, const float *radius, int size,
                                                  int blend, const float *planes, const float *grad_img, float *grad_pts, float *grad_col,
                                                  void *stream)
{
    using namespace genpc;
    const char *fn = "genpc_render_points_ragged_backward";
    RenderRaggedAsk ask;
    ask.s = s; ask.off = off; ask.radius = radius; ask.size = size; ask.blend = blend; ask.backward = true;
    ask.pts = pts != nullptr; ask.planes = planes != nullptr; ask.grad_img = grad_img != nullptr; ask.grad_pts = grad_pts != nullptr;
    const RenderRaggedPlan plan = render_ragged_plan(ask);
    if (plan.refuse) return render_ragged_refuse(fn, plan);
    if (plan.nothing) return 1;
    hipStream_t st = (hipStream_t)stream;
    float *W1;
    float4 *W4;
    int *doff;
    float *dradius;
    WsLayout L;
    L.add(doff, plan.table_ints);
    L.add(dradius, plan.table_floats);
    L.add(W1, plan.w_pixels);
    L.add(W4, plan.w_pixels);
    if (!ws_alloc(L, kWsRenderPointsRaggedGrad, st)) return 0;
    if (!render_ragged_tables(plan.s, off, radius, doff, dradius, st)) return 0;
    hipLaunchKernelGGL(render_w_kernel, dim3(plan.g_pix, plan.s), dim3(kQBlock), 0, st, plan.pixels, planes, blend ? 2 : 0, grad_img, W1, W4);
#define GENPC_LAUNCH_RENDER_GRAD_RAGGED(BL, CO)                                                                                          \
    hipLaunchKernelGGL((render_grad_points_ragged_kernel<BL, CO>), dim3((unsigned)plan.grad_blocks), dim3(kQBlock), 0, st, plan.nmax, pts, col, \
                       (const float *)dradius, size, (const float *)W1, (const float4 *)W4, grad_pts, grad_col, plan.gx, plan.s, (const int *)doff)
    if (blend) { if (grad_col) GENPC_LAUNCH_RENDER_GRAD_RAGGED(1, 1); else GENPC_LAUNCH_RENDER_GRAD_RAGGED(1, 0); }
    else { if (grad_col) GENPC_LAUNCH_RENDER_GRAD_RAGGED(0, 1); else GENPC_LAUNCH_RENDER_GRAD_RAGGED(0, 0); }
#undef GENPC_LAUNCH_RENDER_GRAD_RAGGED
    return check(hipGetLastError(), "render_points_ragged_backward launch") ? 1 : 0;
}
