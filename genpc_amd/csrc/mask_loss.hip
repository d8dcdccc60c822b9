// mask_loss.hip -- the silhouette ("mask") loss of compute_loss_function (diff_obj_pose.py:286-336) on the images
// mask_render.hip draws, and its backward through the splat to the pose.
// What follows the render is the reference's own torch code, kept: per-channel statistical normalisation,
// luminance, sigmoid soft masks, 30 MSE + BCE + 10 Dice (:204-217,261-278,238-259,304-311) -- restated in
// oracle/genpc_oracle_geom.c, pinned there to the reference's own code (tests/golden/ref_py_mask_loss.npz) and to torch autograd.
//   mask_ref_kernel      the reference image's statistics and soft mask, once per call
//   mask_sums_kernel     pixels over many blocks: the 22 sums the loss and its gradient need
//   mask_w_kernel        d loss / d I_ch per pixel folded with the splat's own derivative into the five
//                        per-pixel weights the backward gather needs; the loss itself
//   mask_grad_kernel     one thread per point: gathers the weights over the pixels it covers, chains
//                        through (u, v, rho) to the point and on to (R, s, t): same 13 accumulators as
//                        the Chamfer gradient
// mask_step = the splat + mask_step_backward (sums, weights, gather); genpc_mask_backward_probe runs the latter on a caller's planes
// (tests/test_gpu_mask_backward_probe.py: weights per pixel and sums per point against tests/mask_loss_ref.py).
#include "mask.h"
#include "../../include/genpc_hip.h"

#include <algorithm>

namespace genpc {

constexpr int kMLThreads = 1024;

// block-wide sums of up to four doubles (all threads get the totals)
__device__ __forceinline__ void block_sum4(double (&x)[4], double (*red)[kMLThreads / kWave])
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double y = wave_sum63(x[k]);
        if (lane == kWave - 1) red[k][wave] = y;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        double y = 0.0;
        for (int w = 0; w < kMLThreads / kWave; w++) y += red[k][w];
        x[k] = y;
    }
    __syncthreads();
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

// compute_soft_mask (diff_obj_pose.py:261-278): sigmoid((luminance - 0.1) / 0.05), float32 like the reference
__device__ __forceinline__ float soft_mask(float r, float g, float b)
{
    const float lum = kLumR * r + kLumG * g + kLumB * b;
    return sigmoidf((lum - 0.1f) / 0.05f);
}

// Reference image of a scan (once per call; one block per scan): per-channel mean and unbiased std of the
// image (normalize_images, :208-209), the soft mask m_ref = soft_mask(I_ref) into mref[P] and
// stats[8] = mean[3], std[3], sum m_ref, 0.
__global__ __launch_bounds__(kMLThreads) void mask_ref_kernel(int S, const float *__restrict__ planes, int direct,
                                                              float *__restrict__ mref, float *__restrict__ stats)
{
    __shared__ double red[4][kMLThreads / kWave];
    const int e = blockIdx.x, P = S * S;
    planes += (size_t)e * 5 * P;
    mref += (size_t)e * P;
    stats += (size_t)e * 8;
    double a[4] = {0, 0, 0, 0};
    for (int q = threadIdx.x; q < P; q += kMLThreads) {
        const PxImg px = load_pixel(planes, P, q, direct);
        a[0] += (double)px.I[0]; a[1] += (double)px.I[1]; a[2] += (double)px.I[2];
    }
    block_sum4(a, red);
    const double mu[3] = {a[0] / P, a[1] / P, a[2] / P};
    double b[4] = {0, 0, 0, 0};
    for (int q = threadIdx.x; q < P; q += kMLThreads) {
        const PxImg px = load_pixel(planes, P, q, direct);
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const double dd = (double)px.I[ch] - mu[ch];
            b[ch] += dd * dd;
        }
        const float m = soft_mask(px.I[0], px.I[1], px.I[2]);
        b[3] += (double)m;
        mref[q] = m;
    }
    block_sum4(b, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            stats[ch] = (float)mu[ch];
            stats[3 + ch] = (float)sqrt(b[ch] / (P - 1));
        }
        stats[6] = (float)b[3];
        stats[7] = 0.0f;
    }
}

// per-channel statistics of the posed cloud's image from the sums in accum[16..21], and the reference's
struct MaskStats {
    float muf[3], k[3], murf[3];
    double sd[3], mu[3], sdr[3];
};

__device__ __forceinline__ MaskStats mask_image_stats(const double *accum, const float *stats, int P)
{
    MaskStats o;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const double mu = accum[16 + ch] / P;
        double var = (accum[19 + ch] - (double)P * mu * mu) / (P - 1);
        var = var > 0.0 ? var : 0.0;
        o.mu[ch] = mu;
        o.sd[ch] = sqrt(var);
        o.sdr[ch] = (double)stats[3 + ch];
        o.k[ch] = (float)((o.sdr[ch] + 1e-6) / (o.sd[ch] + 1e-6));
        o.muf[ch] = (float)mu;
        o.murf[ch] = stats[ch];
    }
    return o;
}

// the per-pixel quantities every pass needs
struct MaskPx {
    float m, mr;
    float spc[3];            // d m / d I'_ch (normalised image): 0 where the clamp or the saturated sigmoid cuts the gradient
    float lm, l1m, dmb;      // clamped logs; d (30 MSE + BCE) / d m * P
};

__device__ __forceinline__ MaskPx mask_pixel(const float *I, float mr, const MaskStats &st)
{
    MaskPx o;
    float xn[3];
    bool inside[3];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const float x0 = (I[ch] - st.muf[ch]) * st.k[ch] + st.murf[ch];
        inside[ch] = x0 > 0.0f && x0 < 1.0f;
        xn[ch] = fminf(fmaxf(x0, 0.0f), 1.0f);
    }
    o.m = soft_mask(xn[0], xn[1], xn[2]);
    o.mr = mr;
    const float lm = logf(o.m), l1m = logf(1.0f - o.m);
    o.lm = fmaxf(lm, -100.0f);
    o.l1m = fmaxf(l1m, -100.0f);
    const float sp = o.m * (1.0f - o.m) * 20.0f;
    o.spc[0] = inside[0] ? sp * kLumR : 0.0f;
    o.spc[1] = inside[1] ? sp * kLumG : 0.0f;
    o.spc[2] = inside[2] ? sp * kLumB : 0.0f;
    float db = 0.0f;
    if (lm > -100.0f) db -= mr / o.m;
    if (l1m > -100.0f) db += (1.0f - mr) / (1.0f - o.m);
    o.dmb = 60.0f * (o.m - mr) + db;
    return o;
}

// grid (blocks, b): accum[16..21] += sum I_ch, sum I_ch^2 of a five-plane image read as `direct` says (the splat does this for its own)
__global__ __launch_bounds__(kQBlock) void mask_image_sums_kernel(int P, const float *__restrict__ planes, int direct,
                                                                  double *__restrict__ accum)
{
    __shared__ double red[6][kQBlock / kWave];
    const int e = blockIdx.y;
    planes += (size_t)e * 5 * P;
    accum += (size_t)e * kAcc;
    double a[6] = {0, 0, 0, 0, 0, 0};
    for (int q = blockIdx.x * kQBlock + threadIdx.x; q < P; q += gridDim.x * kQBlock) {
        const PxImg px = load_pixel(planes, P, q, direct);
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const double I = (double)px.I[ch];
            a[ch] += I;
            a[3 + ch] += I * I;
        }
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const double x = wave_sum63(a[i]);
        if (lane == kWave - 1) red[i][wave] = x;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        double x = 0.0;
#pragma unroll
        for (int w2 = 0; w2 < kQBlock / kWave; w2++) x += red[threadIdx.x][w2];
        atomicAdd(&accum[16 + threadIdx.x], x);
    }
}

// grid (blocks, b).  accum[22..25] += mse, bce, intersection, sum m, and per channel, with g1 = dmb spc / P,
// g2 = mr spc, g3 = spc:  accum[26 + 6 ch ..] += sum g1, sum g2, sum g3, sum g1 (I - mu), sum g2 (I - mu),
// sum g3 (I - mu)  -- the Dice term's share of G is (dice_a g2 + dice_b g3) with coefficients only known
// after this pass.
constexpr int kMaskSums = 22;
__global__ __launch_bounds__(kQBlock) void mask_sums_kernel(int S, const float *__restrict__ planes, int direct,
                                                            const float *__restrict__ mref,
                                                            const float *__restrict__ stats, double *__restrict__ accum)
{
    __shared__ double red[kMaskSums][kQBlock / kWave];
    const int e = blockIdx.y, P = S * S;
    planes += (size_t)e * 5 * P;
    mref += (size_t)e * P;
    stats += (size_t)e * 8;
    accum += (size_t)e * kAcc;
    const MaskStats st = mask_image_stats(accum, stats, P);
    const float invP = 1.0f / (float)P;
    double a[kMaskSums];
#pragma unroll
    for (int i = 0; i < kMaskSums; i++) a[i] = 0.0;
    for (int q = blockIdx.x * kQBlock + threadIdx.x; q < P; q += gridDim.x * kQBlock) {
        const PxImg im = load_pixel(planes, P, q, direct);
        const MaskPx px = mask_pixel(im.I, mref[q], st);
        a[0] += (double)((px.m - px.mr) * (px.m - px.mr));
        a[1] += (double)(-(px.mr * px.lm + (1.0f - px.mr) * px.l1m));
        a[2] += (double)(px.m * px.mr);
        a[3] += (double)px.m;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const double g1 = (double)(px.dmb * px.spc[ch] * invP), g2 = (double)(px.mr * px.spc[ch]), g3 = (double)px.spc[ch];
            const double dI = (double)im.I[ch] - st.mu[ch];
            a[4 + 6 * ch + 0] += g1; a[4 + 6 * ch + 1] += g2; a[4 + 6 * ch + 2] += g3;
            a[4 + 6 * ch + 3] += g1 * dI; a[4 + 6 * ch + 4] += g2 * dI; a[4 + 6 * ch + 5] += g3 * dI;
        }
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < kMaskSums; i++) {
        const double x = wave_sum63(a[i]);
        if (lane == kWave - 1) red[i][wave] = x;
    }
    __syncthreads();
    if (threadIdx.x < kMaskSums) {
        double x = 0.0;
#pragma unroll
        for (int w2 = 0; w2 < kQBlock / kWave; w2++) x += red[threadIdx.x][w2];
        atomicAdd(&accum[22 + threadIdx.x], x);
    }
}

// What the backward gather needs per image besides the pixel itself: the Dice term's two coefficients and, per channel, the
// mean of G and the factor of the standard deviation's own derivative (mask_w_kernel's prologue; the fused gather's too)
struct MaskCoef {
    float dice_a, dice_b, meanG[3], kk[3], invP, mask_weight;
};

__device__ __forceinline__ MaskCoef mask_coefficients(const double *accum, const float *stats, const MaskStats &st, int P, float mask_weight)
{
    MaskCoef o;
    const double den = accum[25] + (double)stats[6] + 1e-6, num = 2.0 * accum[24] + 1e-6;
    o.dice_a = (float)(-20.0 / den);
    o.dice_b = (float)(10.0 * num / (den * den));
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const double *s = accum + 26 + 6 * ch;
        const double sG = s[0] + (double)o.dice_a * s[1] + (double)o.dice_b * s[2];
        const double sGd = s[3] + (double)o.dice_a * s[4] + (double)o.dice_b * s[5];
        o.meanG[ch] = (float)(sG / P);
        const double sd = st.sd[ch];
        o.kk[ch] = sd > 0.0 ? (float)((st.sdr[ch] + 1e-6) / ((sd + 1e-6) * (sd + 1e-6)) / ((P - 1) * sd) * sGd) : 0.0f;
    }
    o.invP = 1.0f / (float)P;
    o.mask_weight = mask_weight;
    return o;
}

__device__ __forceinline__ double mask_loss_value(const double *accum, const float *stats, int P)
{
    const double den = accum[25] + (double)stats[6] + 1e-6, num = 2.0 * accum[24] + 1e-6;
    return 30.0 * accum[22] / P + accum[23] / P + 10.0 * (1.0 - num / den);
}

// the weights of pixel q (mask_w_kernel's body; the fused gather evaluates it per gathered pixel: same arithmetic, same bits)
__device__ __forceinline__ void mask_w_pixel(const float *__restrict__ planes, const float *__restrict__ mref, int P, int q, int direct,
                                             const MaskStats &st, const MaskCoef &cf, float &w1, float4 &w4)
{
    const PxImg im = load_pixel(planes, P, q, direct);
    const MaskPx px = mask_pixel(im.I, mref[q], st);
    const float Gm = px.dmb * cf.invP + cf.dice_a * px.mr + cf.dice_b;
    float dI[3];
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
        dI[ch] = cf.mask_weight * (st.k[ch] * (Gm * px.spc[ch] - cf.meanG[ch]) - cf.kk[ch] * (im.I[ch] - st.muf[ch]));
    if (direct == 2) {
        // blend 1: I_ch = N'_ch / D', N' and D' sums of w_i = a_i e'_i:  d loss / d w_i = W4.xyz . c_i - W4.w; the gather
        // multiplies by e'_i = exp(z_i / gamma - m), so W1 carries the pixel's m
        const float sI = dI[0] * im.I[0] + dI[1] * im.I[1] + dI[2] * im.I[2];
        w1 = im.T;
        w4 = make_float4(im.iD * dI[0], im.iD * dI[1], im.iD * dI[2], im.iD * sI);
    } else if (direct) {
        w4 = make_float4(dI[0], dI[1], dI[2], 0.0f);
        w1 = 0.0f;
    } else {
        const float sA = dI[0] * im.A[0] + dI[1] * im.A[1] + dI[2] * im.A[2];
        const float od = im.O * im.iD;
        w1 = im.T * sA;
        w4 = make_float4(od * dI[0], od * dI[1], od * dI[2], od * sA);
    }
}

// grid (blocks, b): with dI_ch = mask_weight * d mask_loss / d I_ch, the five weights of the backward gather
//   W1 = T sum_ch dI_ch A_ch     (d O / d a_i = T / (1 - a_i))
//   W4 = (O / D) (dI_r, dI_g, dI_b, sum_ch dI_ch A_ch)     (d A_ch / d a_i = (c_i,ch - A_ch) / D)
// so that d loss / d a_i = W1 / (1 - a_i) + W4.xyz . c_i - W4.w.  direct: W4.xyz = dI itself.
// Block 0 adds mask_weight * mask_loss to accum[15].
__global__ __launch_bounds__(kQBlock) void mask_w_kernel(int S, const float *__restrict__ planes, int direct,
                                                         const float *__restrict__ mref,
                                                         const float *__restrict__ stats, float mask_weight,
                                                         float *__restrict__ W1, float4 *__restrict__ W4,
                                                         double *__restrict__ accum)
{
    const int e = blockIdx.y, P = S * S;
    planes += (size_t)e * 5 * P;
    mref += (size_t)e * P;
    W1 += (size_t)e * P;
    W4 += (size_t)e * P;
    stats += (size_t)e * 8;
    accum += (size_t)e * kAcc;
    const MaskStats st = mask_image_stats(accum, stats, P);
    const MaskCoef cf = mask_coefficients(accum, stats, st, P, mask_weight);
    for (int q = blockIdx.x * kQBlock + threadIdx.x; q < P; q += gridDim.x * kQBlock) {
        float w1;
        float4 w4;
        mask_w_pixel(planes, mref, P, q, direct, st, cf, w1, w4);
        W1[q] = w1;
        W4[q] = w4;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) accum[15] += (double)mask_weight * mask_loss_value(accum, stats, P);
}

// 1-D grid of gx * nb blocks (xcd_block): gradient of the mask term with respect to (R, s, t), into accum[0..12].
// FUSEW (round 6): the per-pixel weights are not read from W1 / W4 but evaluated where they are gathered, from the image's
// planes and the reference mask with mask_w_kernel's own arithmetic (mask_w_pixel: same bits) -- the alignment loop's step is
// one launch shorter (mask_w_kernel: 13 us of a 128 us step for 50 k pixels per image); block 0 of an image adds the loss.
template <int kGradSub, int BLEND, int FUSEW = 0>
__global__ __launch_bounds__(kQBlock) void mask_grad_kernel(int n, const float *__restrict__ v,
                                                            const float *__restrict__ col,
                                                            const float *__restrict__ center, int cstride,
                                                            const float *__restrict__ params, int pstride, float radius,
                                                            int S, const float *__restrict__ W1,
                                                            const float4 *__restrict__ W4, double *__restrict__ accum,
                                                            int gx, int nb, const float *__restrict__ planes = nullptr,
                                                            const float *__restrict__ mref = nullptr,
                                                            const float *__restrict__ stats = nullptr, float mask_weight = 0.0f,
                                                            PoseGradArgs pg = PoseGradArgs{}, const int *__restrict__ off = nullptr)
{
    __shared__ double red[15][kQBlock / kWave];
    // (one stream, full objective: the Chamfer half's gradient rides along as the launch's last blocks -- a launch less per step)
    if (pg.gx > 0 && (int)blockIdx.x >= gx * nb) {
        const int r = (int)blockIdx.x - gx * nb;
        pose_grad_body(r % pg.gx, pg.gx, r / pg.gx, pg.nc, pg.v, pg.center, pg.cstride, pg.params, pg.pstride, pg.np, pg.partial, pg.d1, pg.i1,
                       pg.d2, pg.i2, pg.cd_weight, pg.accum, red, pg.coff, pg.poff);
        return;
    }
    const XcdBlock xb = xcd_block(gx, nb);
    const int e = xb.e;
    const PoseSpan sp = pose_span(off, e, n);
    n = sp.n;
    // a short element of a ragged call: the whole block leaves (block 0 of an element always has points, and it is the one that adds the loss)
    if (off && xb.x * (kQBlock / kGradSub) >= n) return;
    v += sp.base * 3;
    if (col) col += sp.base * 3;
    const int PP = S * S;
    if (!FUSEW) {
        W1 += (size_t)e * PP;
        W4 += (size_t)e * PP;
    }
    center += (size_t)e * cstride;
    params += (size_t)e * pstride;
    accum += (size_t)e * kAcc;
    MaskStats mst = {};
    MaskCoef mcf = {};
    if (FUSEW) {
        planes += (size_t)e * 5 * PP;
        mref += (size_t)e * PP;
        stats += (size_t)e * 8;
        mst = mask_image_stats(accum, stats, PP);
        mcf = mask_coefficients(accum, stats, mst, PP, mask_weight);
    }
    constexpr int kMode = BLEND ? 2 : 0;
    float R[9];
    rot6d_to_matrix(params, R);
    const float s = expf(params[9]);
    const float c[3] = {center[0], center[1], center[2]};
    const float t[3] = {params[6], params[7], params[8]};
    const float hs = 0.5f * S;
    double a[13];
#pragma unroll
    for (int k = 0; k < 13; k++) a[k] = 0.0;
    // kGradSub lanes share a point: each takes every kGradSub-th row of the point's pixel box, the partial sums meet
    // by shuffles and the first lane does the chain rule.  One scan: 8 lanes (one thread per point leaves 64 blocks
    // for 16384 points and a 64-pixel serial loop per thread: 21 us of a 109 us step -> 102); several scans in
    // lock-step fill the chip with one thread per point, and the idle lanes of the 8-lane form cost 7 % there.
    const int sub = threadIdx.x & (kGradSub - 1);
    const int per_block = kQBlock / kGradSub;
    for (int j0 = xb.x * per_block; j0 < n; j0 += gx * per_block) {
        const int j = j0 + threadIdx.x / kGradSub;
        const bool live = j < n;
        const int jj = live ? j : n - 1;
        const float vx = v[(size_t)jj * 3 + 0], vy = v[(size_t)jj * 3 + 1], vz = v[(size_t)jj * 3 + 2];
        float cr = 1.0f, cg = 1.0f, cb = 1.0f;
        if (col) { cr = col[(size_t)jj * 3 + 0]; cg = col[(size_t)jj * 3 + 1]; cb = col[(size_t)jj * 3 + 2]; }
        float p[3];
        pose_point(R, s, c, t, vx, vy, vz, p);
        const SplatPt q = splat_project(p, radius, hs);
        const bool ok = live && q.ok;
        const int c0 = max((int)floorf(q.u - q.rho - 0.5f), 0), c1 = min((int)ceilf(q.u + q.rho - 0.5f), S - 1);
        const int r0 = max((int)floorf(q.v - q.rho - 0.5f), 0), r1 = min((int)ceilf(q.v + q.rho - 0.5f), S - 1);
        const float ir2 = 1.0f / (q.rho * q.rho);
        float gu = 0.0f, gv = 0.0f, gr = 0.0f, gz = 0.0f;
        const float ze = pulsar_ze(q.zv);
        if (ok) {
            // rows with an empty chord skipped, a row over its chord +- a pixel, the hardware reciprocal for 1 / (1 - av)
            const float rho2 = q.rho * q.rho;
            for (int r = r0 + sub; r <= r1; r += kGradSub) {
                const float dy = (float)r + 0.5f - q.v;
                const float h2 = rho2 - dy * dy;
                if (h2 < -1e-5f * rho2) continue;
                const float h = sqrtf(fmaxf(h2, 0.0f));
                const int ca = max((int)floorf(q.u - h - 0.5f), c0), cz = min((int)ceilf(q.u + h - 0.5f), c1);
                for (int cc = ca; cc <= cz; cc++) {
                    const float dx = (float)cc + 0.5f - q.u;
                    const float d2 = dx * dx + dy * dy;
                    const float av = 1.0f - d2 * ir2;
                    if (BLEND) {
                        if (av <= 0.0f) continue;
                        float4 w4;
                        float w1;
                        if (FUSEW) mask_w_pixel(planes, mref, PP, r * S + cc, kMode, mst, mcf, w1, w4);
                        else { w4 = W4[(size_t)r * S + cc]; w1 = W1[(size_t)r * S + cc]; }
                        const float w = ((cr * w4.x + cg * w4.y) + (cb * w4.z - w4.w)) * __expf(ze - w1);
                        gz += w * fminf(av, kMaskAmax);
                        if (av >= kMaskAmax) continue;
                        gu += w * dx;
                        gv += w * dy;
                        gr += w * d2;
                        continue;
                    }
                    if (av <= 0.0f || av >= kMaskAmax) continue;      // outside the disc / clamped: no gradient
                    float4 w4;
                    float w1;
                    if (FUSEW) mask_w_pixel(planes, mref, PP, r * S + cc, kMode, mst, mcf, w1, w4);
                    else { w4 = W4[(size_t)r * S + cc]; w1 = W1[(size_t)r * S + cc]; }
                    const float w = w1 * __builtin_amdgcn_rcpf(1.0f - av) + ((cr * w4.x + cg * w4.y) + (cb * w4.z - w4.w));
                    gu += w * dx;
                    gv += w * dy;
                    gr += w * d2;
                }
            }
        }
        if (kGradSub == 8) {
            // the eight lanes of a point: quads by permutation, then the mirror image within the eight (DPP: no LDS round trips)
            gu += dpp_or_zero<0xB1>(gu); gu += dpp_or_zero<0x4E>(gu); gu += dpp_or_zero<0x141>(gu);
            gv += dpp_or_zero<0xB1>(gv); gv += dpp_or_zero<0x4E>(gv); gv += dpp_or_zero<0x141>(gv);
            gr += dpp_or_zero<0xB1>(gr); gr += dpp_or_zero<0x4E>(gr); gr += dpp_or_zero<0x141>(gr);
            if (BLEND) { gz += dpp_or_zero<0xB1>(gz); gz += dpp_or_zero<0x4E>(gz); gz += dpp_or_zero<0x141>(gz); }
        } else {
#pragma unroll
            for (int off = kGradSub / 2; off > 0; off >>= 1) {
                gu += __shfl_xor(gu, off, kWave);
                gv += __shfl_xor(gv, off, kWave);
                gr += __shfl_xor(gr, off, kWave);
                if (BLEND) gz += __shfl_xor(gz, off, kWave);
            }
        }
        if (!ok || sub != 0) continue;
        gu *= 2.0f * ir2; gv *= 2.0f * ir2; gr *= 2.0f * ir2 / q.rho;
        const double iz = 1.0 / (double)q.zv;
        const double f4 = (double)hs * kMaskFocal;
        // (blend 1: the weights also depend on the depth, z / gamma = (zfar - Zv) kPulsarZeK)
        const double gzv = (double)gu * (-f4 * p[0] * iz * iz) + (double)gv * (f4 * p[1] * iz * iz) + (double)gr * (-(double)q.rho * iz) +
                           (BLEND ? -(double)gz * (double)kPulsarZeK : 0.0);
        const double g[3] = {(double)gu * f4 * iz, -(double)gv * f4 * iz, -gzv};
        const double l[3] = {(double)(vx - c[0]), (double)(vy - c[1]), (double)(vz - c[2])};
#pragma unroll
        for (int r = 0; r < 3; r++) {
            a[10 + r] += g[r];
#pragma unroll
            for (int qq = 0; qq < 3; qq++) a[r * 3 + qq] += g[r] * (double)s * l[qq];
            a[9] += g[r] * ((double)R[r * 3 + 0] * l[0] + (double)R[r * 3 + 1] * l[1] + (double)R[r * 3 + 2] * l[2]);
        }
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 13; k++) {
        const double x = wave_sum63(a[k]);
        if (lane == kWave - 1) red[k][wave] = x;
    }
    __syncthreads();
    if (threadIdx.x < 13) {
        double x = 0.0;
#pragma unroll
        for (int w2 = 0; w2 < kQBlock / kWave; w2++) x += red[threadIdx.x][w2];
        atomicAdd(&accum[threadIdx.x], x);
    }
    if (FUSEW && xb.x == 0 && threadIdx.x == 0) accum[15] += (double)mask_weight * mask_loss_value(accum, stats, PP);
}

// [P, 3] -> planes 0..2 (genpc_mask_loss's inputs)
__global__ void mask_to_planes_kernel(int P, const float *__restrict__ img, float *__restrict__ planes)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= P) return;
    planes[q] = img[(size_t)q * 3 + 0];
    planes[(size_t)P + q] = img[(size_t)q * 3 + 1];
    planes[2 * (size_t)P + q] = img[(size_t)q * 3 + 2];
}

// genpc_mask_loss's outputs: loss from accum[15], grad[P, 3] from W4.xyz; clears the accumulators
__global__ void mask_loss_out_kernel(int P, const float4 *__restrict__ W4, double *__restrict__ accum,
                                     float *__restrict__ loss_out, float *__restrict__ grad)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (grad && q < P) {
        const float4 w = W4[q];
        grad[(size_t)q * 3 + 0] = w.x;
        grad[(size_t)q * 3 + 1] = w.y;
        grad[(size_t)q * 3 + 2] = w.z;
    }
    if (q == 0) *loss_out = (float)accum[15];
}

int mask_prepare_ref(int b, int np, const float *partial, const float *partial_col, float radius, int S, const MaskScratch &m, hipStream_t st,
                     const int *off)
{
    launch_mask_splat(b, np, partial, partial_col, true, nullptr, 0, nullptr, 0, 0, radius, S, m, nullptr, st, off);
    hipLaunchKernelGGL(mask_ref_kernel, dim3(b), dim3(kMLThreads), 0, st, S, (const float *)m.planes, render_blend() ? 2 : 0, m.mref, m.stats);
    return check(hipGetLastError(), "mask reference launch") ? 1 : 0;
}

// What a silhouette step does once the image of the posed clouds stands in m.planes with its sums in accum[16..21]: the loss's sums,
// the per-pixel weights (unless the gather evaluates them) and the gather.  rad: the radius the image was drawn with.
int mask_step_backward(const MaskStepPlan &plan, int blend, int b, int nc, const float *complete, const float *complete_col,
                       const float *center, int cstride, const float *params, int pstride, float rad, int S, float mask_weight,
                       const MaskScratch &m, double *accum, hipStream_t st, const PoseGradArgs *ride, const int *off)
{
    const int mode = blend ? 2 : 0;
    hipLaunchKernelGGL(mask_sums_kernel, dim3(plan.gs, b), dim3(kQBlock), 0, st, S, (const float *)m.planes, mode, (const float *)m.mref,
                       (const float *)m.stats, accum);
    if (!plan.fuse_w)
        hipLaunchKernelGGL(mask_w_kernel, dim3(plan.gp, b), dim3(kQBlock), 0, st, S, (const float *)m.planes, mode, (const float *)m.mref,
                           (const float *)m.stats, mask_weight, m.W1, m.W4, accum);
    const PoseGradArgs pgx = ride ? *ride : PoseGradArgs{};
#define GENPC_LAUNCH_MASK_GRAD3(SUB, BL, FW)                                                                                         \
    hipLaunchKernelGGL((mask_grad_kernel<SUB, BL, FW>), dim3(lin_grid((long long)nc * SUB) * b + pgx.gx * b), dim3(kQBlock), 0, st, nc, complete, \
                       complete_col, center, cstride, params, pstride, rad, S, (const float *)m.W1, (const float4 *)m.W4, accum,     \
                       lin_grid((long long)nc * SUB), b, (const float *)m.planes, (const float *)m.mref, (const float *)m.stats,      \
                       mask_weight, pgx, off)
#define GENPC_LAUNCH_MASK_GRAD2(SUB, BL) do { if (plan.fuse_w) GENPC_LAUNCH_MASK_GRAD3(SUB, BL, 1); else GENPC_LAUNCH_MASK_GRAD3(SUB, BL, 0); } while (0)
#define GENPC_LAUNCH_MASK_GRAD(SUB) do { if (blend) GENPC_LAUNCH_MASK_GRAD2(SUB, 1); else GENPC_LAUNCH_MASK_GRAD2(SUB, 0); } while (0)
    if (plan.sub8) GENPC_LAUNCH_MASK_GRAD(8);
    else GENPC_LAUNCH_MASK_GRAD(1);
#undef GENPC_LAUNCH_MASK_GRAD3
#undef GENPC_LAUNCH_MASK_GRAD2
#undef GENPC_LAUNCH_MASK_GRAD
    return check(hipGetLastError(), "mask step launch") ? 1 : 0;
}

int mask_step(int b, int nc, const float *complete, const float *complete_col, const float *center, int cstride, const float *params,
              int pstride, float radius, int S, float mask_weight, const MaskScratch &m, double *accum, hipStream_t st, bool projected,
              const PoseGradArgs *ride, const int *off, const MaskStepPlan *shape)
{
    const float rad = 1.1f * radius;      // diff_obj_pose.py:385: the posed cloud is drawn with 1.1 x the radius
    const MaskStepPlan plan = shape ? *shape : mask_step_plan(b, nc, S, radius);      // (every size and choice below, with its reason: pose_plan.h)
    // (the alignment loop projects in its transform launch)
    launch_mask_splat(b, nc, complete, complete_col, !projected, center, cstride, params, pstride, 1, rad, S, m, accum, st, off);
    return mask_step_backward(plan, render_blend(), b, nc, complete, complete_col, center, cstride, params, pstride, rad, S, mask_weight, m,
                              accum, st, ride, off);
}

}  // namespace genpc

GENPC_API int genpc_mask_loss(int size, const float *img, const float *ref, float *loss_out, float *grad, void *stream)
{
    using namespace genpc;
    if (size <= 1) return -1;
    hipStream_t st = (hipStream_t)stream;
    const int P = size * size;
    double *accum;
    MaskScratch m;
    WsLayout L;
    L.add(accum, 64);          // (kAcc sums in a 512-byte piece)
    m.layout(L, 2, (size_t)P, 1);
    if (!ws_alloc(L, kWsMaskLoss, st)) return 0;
    float *pl_img = m.planes, *pl_ref = m.planes + (size_t)5 * P;
    if (!check(hipMemsetAsync(accum, 0, kAcc * sizeof(double), st), "hipMemsetAsync(accum)")) return 0;
    const int g256 = ceil_div(P, 256), gp = lin_grid(P);
    hipLaunchKernelGGL(mask_to_planes_kernel, dim3(g256), dim3(256), 0, st, P, img, pl_img);
    hipLaunchKernelGGL(mask_to_planes_kernel, dim3(g256), dim3(256), 0, st, P, ref, pl_ref);
    hipLaunchKernelGGL(mask_ref_kernel, dim3(1), dim3(kMLThreads), 0, st, size, (const float *)pl_ref, 1, m.mref, m.stats);
    hipLaunchKernelGGL(mask_image_sums_kernel, dim3(gp, 1), dim3(kQBlock), 0, st, P, (const float *)pl_img, 1, accum);
    hipLaunchKernelGGL(mask_sums_kernel, dim3(gp, 1), dim3(kQBlock), 0, st, size, (const float *)pl_img, 1, (const float *)m.mref,
                       (const float *)m.stats, accum);
    hipLaunchKernelGGL(mask_w_kernel, dim3(gp, 1), dim3(kQBlock), 0, st, size, (const float *)pl_img, 1, (const float *)m.mref,
                       (const float *)m.stats, 1.0f, m.W1, m.W4, accum);
    hipLaunchKernelGGL(mask_loss_out_kernel, dim3(g256), dim3(256), 0, st, P, (const float4 *)m.W4, accum, loss_out, grad);
    return check(hipGetLastError(), "mask_loss launch") ? 1 : 0;
}

GENPC_API int genpc_mask_backward_probe(int S, int blend, int sub8, int fuse_w, const float *planes, const float *ref_img, int n,
                                        const float *pts, const float *col, const float *center, const float *params, float radius,
                                        float mask_weight, double *accum_out, float *W1_out, float *W4_out, void *stream)
{
    using namespace genpc;
    if (S <= 1 || n < 1 || !planes || !ref_img || !pts || !center || !params || !accum_out) return -1;
    hipStream_t st = (hipStream_t)stream;
    const int P = S * S;
    double *accum;
    MaskScratch m;
    WsLayout L;
    L.add(accum, 64);          // (genpc_mask_loss's layout: image 0 the posed cloud's planes, image 1 the reference's)
    m.layout(L, 2, (size_t)P, 1);
    if (!ws_alloc(L, kWsMaskLoss, st)) return 0;
    float *pl_ref = m.planes + (size_t)5 * P;
    if (!check(hipMemsetAsync(accum, 0, kAcc * sizeof(double), st), "hipMemsetAsync(accum)")) return 0;
    if (!check(hipMemcpyAsync(m.planes, planes, (size_t)5 * P * sizeof(float), hipMemcpyDeviceToDevice, st), "hipMemcpyAsync(planes)")) return 0;
    MaskStepPlan plan{};
    plan.gp = lin_grid(P);
    plan.gs = std::min(plan.gp, 48);
    plan.fuse_w = fuse_w != 0;
    plan.sub8 = sub8 != 0;
    hipLaunchKernelGGL(mask_to_planes_kernel, dim3(ceil_div(P, 256)), dim3(256), 0, st, P, ref_img, pl_ref);
    hipLaunchKernelGGL(mask_ref_kernel, dim3(1), dim3(kMLThreads), 0, st, S, (const float *)pl_ref, 1, m.mref, m.stats);
    hipLaunchKernelGGL(mask_image_sums_kernel, dim3(plan.gp, 1), dim3(kQBlock), 0, st, P, (const float *)m.planes, blend ? 2 : 0, accum);
    if (!mask_step_backward(plan, blend, 1, n, pts, col, center, 0, params, 0, radius, S, mask_weight, m, accum, st, nullptr, nullptr)) return 0;
    if (!check(hipMemcpyAsync(accum_out, accum, 16 * sizeof(double), hipMemcpyDeviceToDevice, st), "hipMemcpyAsync(accum_out)")) return 0;
    if (!plan.fuse_w) {
        if (W1_out && !check(hipMemcpyAsync(W1_out, m.W1, (size_t)P * sizeof(float), hipMemcpyDeviceToDevice, st), "hipMemcpyAsync(W1)")) return 0;
        if (W4_out && !check(hipMemcpyAsync(W4_out, m.W4, (size_t)P * sizeof(float4), hipMemcpyDeviceToDevice, st), "hipMemcpyAsync(W4)")) return 0;
    }
    return 1;
}
