// mask.h -- what the renderer (mask_render.hip), the silhouette loss (mask_loss.hip) and the loop's fused transform
// (pose.hip pose_transform_project_kernel) share of the mask term: the renderer's constants, projection and tile binning, the
// five-plane image, the XCD block map, the term's scratch, and the host entry points of the two files.
// The splat is defined at the top of mask_render.hip, the loss at the top of mask_loss.hip.
#pragma once
#include "pose.h"

namespace genpc {

constexpr int kMaskTile = 16;
constexpr int kSplatBlock = 1024;  // 16 waves per tile: a wave per point leaves long dependent chains, four waves per SIMD hide them
constexpr int kSplatPer = 16;      // points per thread and round of the splat (16384 points per round)
constexpr int kSplatList = 1024;   // in-tile points drawn per fill of the LDS list (full-scan path; the list path holds a whole tile list: kTileCap)
constexpr float kMaskAmax = 0.999f;
// (the camera -- kMaskFocal, kMaskEyeZ, kMaskZnear, kMaskZfar -- is pose_plan.h's: the host's plan sizes a disc with it)
constexpr float kLumR = 0.299f, kLumG = 0.587f, kLumB = 0.114f;      // compute_soft_mask, diff_obj_pose.py:273
// Blend 1 = Pulsar's published blending function (Lassner & Zollhoefer, CVPR 2021, eq. 1-2) with the reference's arguments
// (diff_obj_pose.py:126-131,428-433: gamma 1e-2, znear 1e-4, zfar 5, bg 0; opacity 1): a softmax in depth over the discs
// covering a pixel,  I_ch = sum_i a_i e_i c_i,ch / (B + sum_i a_i e_i),  e_i = exp(z_i / gamma),  z_i = (zfar - Zv_i) / (zfar -
// znear),  B = exp(eps / gamma), eps = 1e-10 -- restated, with what is from memory marked, in oracle/genpc_oracle_geom.c and
// pinned there to torch autograd.  The image is kept as five planes like blend 0's: the exponent m every weight of the pixel
// is taken relative to (max(eps, max_i z_i) / gamma), D' = B e^-m + sum a e', N'_ch = sum a e' c_ch with e' = exp(z_i / gamma - m).
constexpr float kPulsarGamma = 1e-2f, kPulsarEps = 1e-10f;
constexpr float kPulsarZe0 = kPulsarEps / kPulsarGamma;                                  // the background's exponent
constexpr float kPulsarZeK = 1.0f / ((kMaskZfar - kMaskZnear) * kPulsarGamma);           // z / gamma = (zfar - Zv) * kPulsarZeK
__device__ __forceinline__ float pulsar_ze(float zv) { return (kMaskZfar - zv) * kPulsarZeK; }

struct SplatPt {
    float u, v, rho, zv;
    bool ok;
};

__device__ __forceinline__ SplatPt splat_project(const float *p, float radius, float hs)
{
    SplatPt o;
    o.zv = kMaskEyeZ - p[2];
    o.ok = o.zv > kMaskZnear && o.zv < kMaskZfar;
    const float iz = 1.0f / o.zv;
    o.u = hs * (1.0f + kMaskFocal * p[0] * iz);
    o.v = hs * (1.0f - kMaskFocal * p[1] * iz);
    o.rho = hs * kMaskFocal * radius * iz;
    return o;
}

// Per-tile index lists (filled by the projection kernels, read and reset by mask_splat_kernel): bins = { count[b][tiles],
// idx[b][tiles][kTileCap] }.  A point goes to every tile its disc's bounding box touches -- THE test of the splat kernel, so
// a tile's list is exactly its hit set; a tile with more than kSplatCap hits (the count keeps counting) is drawn by the
// full scan.  (Every block used to read all projected points of its image: 205 MB of L2 reads per launch of four
// starts, 43 k ticks for an empty tile.)
constexpr int kTileCap = 8192;            // entries a tile's list holds (a small object: 16384 points over a dozen tiles; 4096: 72.8 ms per call, 8192: 60.8)
constexpr int kSplatCap = 1024;          // the splat takes lists up to this length (one entry per thread, one fill)
constexpr int kRankWords = 2048;         // bitmap ranks in the splat: images of up to 65536 points
constexpr int kRankByCount = 256;        // lists up to this length are ranked by counting
constexpr int kBinTiles = 1024;          // tiles per image the block-level histogram holds (S <= 512); larger images: no bins
constexpr int kBinPer = 4;               // tiles a listed disc may touch (entries carry the slot in two bits)

// f(tile) for every tile the disc's bounding box touches, in (row, column) order -- mask_splat_kernel's test, verbatim
template <class F>
__device__ __forceinline__ void for_each_tile(int S, float u, float v, float rho, F f)
{
    const int T = (S + kMaskTile - 1) / kMaskTile;
    int tx_lo = (int)floorf((u - rho) / (float)kMaskTile) - 1, tx_hi = (int)floorf((u + rho) / (float)kMaskTile) + 1;
    int ty_lo = (int)floorf((v - rho) / (float)kMaskTile) - 1, ty_hi = (int)floorf((v + rho) / (float)kMaskTile) + 1;
    tx_lo = tx_lo < 0 ? 0 : tx_lo; ty_lo = ty_lo < 0 ? 0 : ty_lo;
    tx_hi = tx_hi > T - 1 ? T - 1 : tx_hi; ty_hi = ty_hi > T - 1 ? T - 1 : ty_hi;
    for (int ty = ty_lo; ty <= ty_hi; ty++)
        for (int tx = tx_lo; tx <= tx_hi; tx++) {
            const int tx0 = tx * kMaskTile, ty0 = ty * kMaskTile;
            const int tx1 = min(S, tx0 + kMaskTile) - 1, ty1 = min(S, ty0 + kMaskTile) - 1;
            if (u + rho >= (float)tx0 && u - rho <= (float)(tx1 + 1) && v + rho >= (float)ty0 && v - rho <= (float)(ty1 + 1)) f(ty * T + tx);
        }
}

// number of tiles a disc touches; slot = position of `tile` among them (-1: not touched)
__device__ __forceinline__ int tile_count(int S, float u, float v, float rho, int tile, int &slot)
{
    int cnt = 0, sl = -1;
    for_each_tile(S, u, v, rho, [&](int t) {
        if (t == tile) sl = cnt;
        cnt++;
    });
    slot = sl;
    return cnt;
}

constexpr int kBinPoison = 1 << 30;      // set in a tile's counter by a disc that is in no list (over more than kBinPer tiles)

// Block-level binning of one point per thread (all threads of the block call it; `valid`: this thread has a point):
// the tile counts of the block's points are first accumulated in LDS, ONE global atomic per (block, tile) reserves the
// block's range in the tile's list, then the threads write their entries: point index * 4 + slot, slot = the position
// of the tile among the point's tiles (the splat reads the index alone).
// (One global atomic per (point, tile) -- 144 k per launch of four starts, 640 on the counter of a crowded tile -- made
// the 5 us projection kernel 50 us.)  A disc over more than kBinPer tiles is listed nowhere and poisons the counters of
// its tiles: the splat draws those by the full scan.
__device__ __forceinline__ void bin_points_block(int *__restrict__ cnt, int *__restrict__ idx, int *s_cnt, int *s_base, int S, bool valid,
                                                 int j, float u, float v, float rho)
{
    const int T = (S + kMaskTile - 1) / kMaskTile, tiles = T * T;
    for (int t = threadIdx.x; t < tiles; t += blockDim.x) s_cnt[t] = 0;
    __syncthreads();
    int my_tile[kBinPer], my_pos[kBinPer], nmine = 0;
    if (valid && rho > 0.0f) {
        int none;
        const int total = tile_count(S, u, v, rho, -1, none);
        if (total <= kBinPer) {
            for_each_tile(S, u, v, rho, [&](int t) {
                if (nmine < kBinPer) {      // (always: keeps the arrays in registers)
                    my_tile[nmine] = t;
                    my_pos[nmine] = atomicAdd(&s_cnt[t], 1);
                    nmine++;
                }
            });
        } else {
            for_each_tile(S, u, v, rho, [&](int t) { atomicOr(&cnt[t], kBinPoison); });
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < tiles; t += blockDim.x) {
        const int c = s_cnt[t];
        s_base[t] = c ? (atomicAdd(&cnt[t], c) & (kBinPoison - 1)) : 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kBinPer; k++) {
        if (k < nmine) {
            const int pos = s_base[my_tile[k]] + my_pos[k];
            if (pos < kTileCap) idx[(size_t)my_tile[k] * kTileCap + pos] = j * 4 + k;
        }
    }
    __syncthreads();
}
__host__ __device__ __forceinline__ size_t bins_tiles(int S)
{
    const size_t T = (size_t)((S + kMaskTile - 1) / kMaskTile);
    return T * T;
}

// The image of a scan is kept as five planes of P = S * S floats: T, D, N_r, N_g, N_b (header comment).
// `direct` = 1 images (genpc_mask_loss: the caller supplies I itself) hold I_r, I_g, I_b in planes 0..2; `direct` = 2: blend 1's
// planes m, D', N'_ch (T carries m; O = 1; A = I = N' / D').
struct PxImg {
    float I[3];
    float T, O, iD;        // exp(L), 1 - exp(L), 1 / D (0 where no disc covers the pixel)
    float A[3];            // N_ch / D
};

__device__ __forceinline__ PxImg load_pixel(const float *__restrict__ pl, int P, int q, int direct)
{
    PxImg o;
    if (direct == 1) {
        o.I[0] = pl[q]; o.I[1] = pl[P + q]; o.I[2] = pl[2 * P + q];
        o.T = 0.0f; o.O = 1.0f; o.iD = 0.0f;
        o.A[0] = o.A[1] = o.A[2] = 0.0f;
        return o;
    }
    const float d = pl[P + q];
    o.T = pl[q];
    if (direct == 2) {
        o.O = 1.0f;
        o.iD = 1.0f / d;          // (the background term keeps D' > 0)
#pragma unroll
        for (int ch = 0; ch < 3; ch++) o.I[ch] = o.A[ch] = pl[(2 + ch) * P + q] * o.iD;
        return o;
    }
    o.O = 1.0f - o.T;
    o.iD = d > 0.0f ? 1.0f / d : 0.0f;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        o.A[ch] = pl[(2 + ch) * P + q] * o.iD;
        o.I[ch] = o.O * o.A[ch];
    }
    return o;
}

// Workgroups go to the 8 XCDs round-robin by linear id, each XCD with its own 4 MB L2.  A 1-D launch of gx blocks for each
// of nb images, mapped so that an image's blocks share as few XCDs as possible: its W planes (1 MB at 224 x 224) are then
// gathered from ONE L2 instead of all eight (32 images in lock-step: 32 MB through every 4 MB L2; measured on the per-point
// gradient: 168 -> 152 us at 32 images, 30.7 -> 29.3 at 4).
struct XcdBlock { int e, x; };
__device__ __forceinline__ XcdBlock xcd_block(int gx, int nb)
{
    const int lin = blockIdx.x, xcd = lin & 7, k = lin >> 3;
    XcdBlock r;
    if ((nb & 7) == 0) {                       // whole images per XCD
        r.e = 8 * (k / gx) + xcd;
        r.x = k % gx;
    } else if (nb < 8 && 8 % nb == 0 && gx % (8 / nb) == 0) {      // 8 / nb XCDs per image
        r.e = xcd % nb;
        r.x = k * (8 / nb) + xcd / nb;
    } else {
        r.e = lin / gx;
        r.x = lin % gx;
    }
    return r;
}

inline int mask_tiles(int S) { const int t = ceil_div(S, kMaskTile); return t * t; }
inline bool use_bins(int S) { return bins_tiles(S) <= (size_t)kBinTiles; }

// scratch of the mask term for b scans of P pixels and up to nmax points (bytes, 256-aligned pieces)
struct MaskScratch {
    float *stats;      // [b, 8]
    float *mref;       // [b, P]
    float *planes;     // [b, 5, P]
    float *W1;         // [b, P]
    float4 *W4;        // [b, P]
    float4 *uvr;       // [b, nmax]
    float *zex;        // [b, nmax] blend 1: the depth exponents of the projected points
    int *bins;         // [b, tiles] counts | [b, tiles, kTileCap] entries (bin_points_block)
    int *clean;        // [b, tiles]: 1 = the tile's pixels hold the background in all five planes (mask_splat_kernel: an empty tile leaves at once)
    size_t clean_bytes;
    size_t bins_count_bytes;
    static size_t side(size_t P) { size_t S = (size_t)sqrt((double)P); while (S * S < P) S++; return S; }
    static size_t bins_ints(int b, size_t P)
    {
        const size_t t = bins_tiles((int)side(P));
        return t <= (size_t)kBinTiles ? (size_t)b * t * (1 + (size_t)kTileCap) : 0;      // (no lists for such an image: use_bins)
    }
    // the pieces, behind whatever L holds already (this object must stay where it is until L is bound)
    void layout(WsLayout &L, int b, size_t P, size_t nmax)
    {
        const size_t tiles = (size_t)b * bins_tiles((int)side(P));
        L.add(stats, (size_t)b * 8);
        L.add(mref, (size_t)b * P);
        L.add(planes, (size_t)b * 5 * P);
        L.add(W1, (size_t)b * P);
        L.add(W4, (size_t)b * P);
        L.add(uvr, (size_t)b * nmax);
        L.add(zex, (size_t)b * nmax);
        L.add(bins, bins_ints(b, P));
        L.add(clean, tiles);
        clean_bytes = tiles * sizeof(int);
        bins_count_bytes = bins_ints(b, P) ? tiles * sizeof(int) : 0;
    }
    // the tile counters are zero between launches (the splat kernel resets what it reads); once per API call for a
    // workspace that is new or was last used with another batch size
    bool zero_bins(hipStream_t st) const
    {
        // (the planes of a fresh call hold anything: no tile is known to be clean)
        if (clean_bytes && !check(hipMemsetAsync(clean, 0, clean_bytes, st), "hipMemsetAsync(tile flags)")) return false;
        return bins_count_bytes == 0 || check(hipMemsetAsync(bins, 0, bins_count_bytes, st), "hipMemsetAsync(tile counters)");
    }
};

// mask_render.hip
// Which blend the images of the mask term are drawn with (genpc_render_tune): 1 Pulsar's blending function, 0 the coverage splat.
int render_blend();
// The launch pair every image of the mask term is drawn with: the b clouds of n points projected (project: unless the caller's
// transform launch did that already; posed != 0: with center / params first, see mask_project_kernel) and splatted with their
// colours into m.planes; accum: the sums of I and I^2 go to the images' accumulators, or null.
// A ragged call (off: the element table of the clouds on the device, pose.h pose_span; n / np / nc then the LARGEST element's count,
// which sizes the launches) packs pts, col, m.uvr and m.zex by that table; the images, bins and flags stay per element.
void launch_mask_splat(int b, int n, const float *pts, const float *col, bool project, const float *center, int cstride, const float *params,
                       int pstride, int posed, float radius, int S, const MaskScratch &m, double *accum, hipStream_t st,
                       const int *off = nullptr);
// mask_loss.hip
// splat of the partial clouds (with their colours) + reference soft masks / statistics (once per call)
int mask_prepare_ref(int b, int np, const float *partial, const float *partial_col, float radius, int S, const MaskScratch &m, hipStream_t st,
                     const int *off = nullptr);
// the launches of the mask term for the current parameters: accum[0..12] += gradient, accum[15] += loss
// (projected: the caller's transform launch projected already; ride: pose_grad's arguments, when its blocks ride in mask_grad's launch;
//  shape: the step's plan when the caller's own plan made it -- a ragged call's, from its totals -- otherwise mask_step_plan of b x nc)
int mask_step(int b, int nc, const float *complete, const float *complete_col, const float *center, int cstride, const float *params,
              int pstride, float radius, int S, float mask_weight, const MaskScratch &m, double *accum, hipStream_t st,
              bool projected = false, const PoseGradArgs *ride = nullptr, const int *off = nullptr, const MaskStepPlan *shape = nullptr);
// mask_step without its splat: the launches that follow it (mask_sums_kernel, mask_w_kernel unless plan.fuse_w, mask_grad_kernel) on
// the image that stands in m.planes, read as `blend` says, with its sums in accum[16..21]; rad: the radius that image was drawn with
// (genpc_mask_backward_probe calls this on caller-built planes)
int mask_step_backward(const MaskStepPlan &plan, int blend, int b, int nc, const float *complete, const float *complete_col,
                       const float *center, int cstride, const float *params, int pstride, float rad, int S, float mask_weight,
                       const MaskScratch &m, double *accum, hipStream_t st, const PoseGradArgs *ride = nullptr, const int *off = nullptr);

}  // namespace genpc
