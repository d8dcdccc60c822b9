// mask_render.hip -- the differentiable colour splat the silhouette ("mask") half of compute_loss_function
// (diff_obj_pose.py:286-336) is drawn with; the loss on its images is mask_loss.hip's.
// The reference compares Pulsar renders (pytorch3d, CUDA only, absent, unpinned) of the partial
// cloud WITH ITS COLOURS (:108-134; load_point_cloud returns vert_col for every input the pipeline
// produces, :136-164) and of the posed complete cloud with its colours (:426-433).  This build defines
// its OWN differentiable colour splat with the reference's camera and radii -- restated with the loss
// in oracle/genpc_oracle_geom.c, whose loss is pinned to the reference's own code
// (tests/golden/ref_py_mask_loss.npz) and whose gradient is pinned to torch autograd:
//   Zv = 3 - z;  u = S/2 (1 + 4 x / Zv);  v = S/2 (1 - 4 y / Zv);  rho = S/2 * 4 * radius / Zv
//   a_i(pixel) = min(0.999, max(0, 1 - |pixel centre - (u, v)|^2 / rho^2))
//   O = 1 - prod_i (1 - a_i);  A_ch = sum_i a_i c_i,ch / sum_i a_i;  I_ch = O A_ch      (background 0)
// (coverage-weighted colour, order-independent: Pulsar's softmax in depth is NOT reproduced by blend 0; blend 1, the default,
// is Pulsar's published blending function: mask.h kPulsarGamma).
//   mask_project_kernel  every point posed (the transform is fused) and projected once: (u, v, rho); the point's
//                        index goes into the list of every tile its disc's bounding box touches (bin_points_block)
//   mask_splat_kernel    one block per 16 x 16 image tile and scan: the points of the tile's list (every point
//                        of the scan when the list overflowed or the image has no lists), in ascending point
//                        order, are put into LDS with their colours, then every pixel (four
//                        threads each) walks the list and accumulates prod (1 - a), a and a c of the discs
//                        covering it, in list order: no atomics on the image.  Writes the five planes
//                        T = prod (1 - a), D = sum a, N_ch = sum a c_ch and adds the tile's sums of
//                        I_ch and I_ch^2 to the scan's accumulators.  (Measured at 16384 points, single
//                        channel: one thread per point walking its own box 634 us per call -- every
//                        wave pays a full box for its one in-tile lane; a wave per point with LDS
//                        float atomics 36 us, 26 of them in the atomics.)
//   mask_image_kernel    the five planes as an [S, S, 3] image (genpc_splat_image)
#include "mask.h"
#include "../../include/genpc_hip.h"

namespace genpc {

// grid (blocks, b): uvr[e, j] = (u, v, rho, 1 / rho^2), rho = -1 for points the camera does not see.
// posed != 0: v is the complete cloud and is posed with params first.
// (the per-tile index lists it fills: mask.h kTileCap)
__global__ __launch_bounds__(kQBlock) void mask_project_kernel(int n, const float *__restrict__ v,
                                                               const float *__restrict__ center, int cstride,
                                                               const float *__restrict__ params, int pstride, int posed,
                                                               float radius, int S, float4 *__restrict__ uvr, int *__restrict__ bins,
                                                               float *__restrict__ zex, const int *__restrict__ off = nullptr)
{
    const int e = blockIdx.y;
    const PoseSpan sp = pose_span(off, e, n);      // (a ragged call: the element's own count, block-uniform like n)
    n = sp.n;
    v += sp.base * 3;
    uvr += sp.base;
    if (zex) zex += sp.base;             // blend 1: the depth exponent z / gamma of every point
    int *bin_cnt = bins ? bins + (size_t)e * bins_tiles(S) : nullptr;
    int *bin_idx = bins ? bins + (size_t)gridDim.y * bins_tiles(S) + (size_t)e * bins_tiles(S) * kTileCap : nullptr;
    float R[9], s = 1.0f, c[3] = {0, 0, 0}, t[3] = {0, 0, 0};
    if (posed) {
        center += (size_t)e * cstride;
        params += (size_t)e * pstride;
        rot6d_to_matrix(params, R);
        s = expf(params[9]);
        c[0] = center[0]; c[1] = center[1]; c[2] = center[2];
        t[0] = params[6]; t[1] = params[7]; t[2] = params[8];
    }
    const float hs = 0.5f * S;
    __shared__ int s_cnt[kBinTiles], s_base[kBinTiles];
    for (int j0 = blockIdx.x * kQBlock; j0 < n; j0 += gridDim.x * kQBlock) {        // (block-uniform: bin_points_block has barriers)
        const int j = j0 + threadIdx.x;
        const bool valid = j < n;
        const int jj = valid ? j : n - 1;
        float p[3] = {v[(size_t)jj * 3 + 0], v[(size_t)jj * 3 + 1], v[(size_t)jj * 3 + 2]};
        if (posed) {
            float o[3];
            pose_point(R, s, c, t, p[0], p[1], p[2], o);
            p[0] = o[0]; p[1] = o[1]; p[2] = o[2];
        }
        const SplatPt q = splat_project(p, radius, hs);
        if (valid) uvr[j] = make_float4(q.u, q.v, q.ok ? q.rho : -1.0f, q.ok ? 1.0f / (q.rho * q.rho) : 0.0f);
        if (valid && zex) zex[j] = pulsar_ze(q.zv);
        if (bin_cnt) bin_points_block(bin_cnt, bin_idx, s_cnt, s_base, S, valid && q.ok, j, q.u, q.v, q.rho);
    }
}

// what a pixel accumulates of one disc that covers it (coverage ac in (0, kMaskAmax], colours cr / cg / cb, depth exponent ze)
template <int BLEND>
__device__ __forceinline__ void splat_fold(float &tr, float &sd, float &sr, float &sg, float &sb, float ac, float cr, float cg, float cb, float ze)
{
    if (BLEND == 0) {
        tr *= 1.0f - ac;
        sd += ac;
        sr += ac * cr;
        sg += ac * cg;
        sb += ac * cb;
    } else {
        // softmax in depth, one pass: tr is the running maximum of the exponents, the sums are relative to it
        if (ze > tr) {
            const float sc = __expf(tr - ze);
            sd *= sc; sr *= sc; sg *= sc; sb *= sc;
            tr = ze;
        }
        const float w = ac * __expf(ze - tr);
        sd += w;
        sr += w * cr;
        sg += w * cg;
        sb += w * cb;
    }
}

// LDS layout of a listed disc.  Blend 0: list = (u, v, 1 / rho^2, red), list_gb = (green, blue).  Blend 1: list = (u, v, 1 / rho^2,
// depth exponent or weight), list_c = (red, green, blue, -) -- still ONE 16-byte read per disc tested and one more per disc that
// covers the pixel (a third, 4-byte read for the exponent made the gather, which is bound by its LDS reads, 30 % slower).
// Blend 1 without an exponential per (pixel, disc): after a fill of the LDS list (list[k].w = the entries' depth exponents) the
// block takes the fill's largest exponent m_f and turns the entries into weights exp(z_k / gamma - m_f) -- ONE exponential
// per listed disc instead of one per pixel it covers (the per-pair form cost 13 us of a 43 us launch, 3.8 ms of a 57 ms
// completed scan) --, every pixel moves its sums to the reference max(its own, m_f) once, and the gather multiplies.
// Exactness is kept by falling back to splat_fold's per-pair form for a fill whose exponents span more than kPulsarSpan (its
// far entries' weights would underflow: a tile that holds points at both ends of the frustum).  All threads of the block call
// it between the fill's barrier and the gather; zlo / zhi: the smallest / largest exponent this thread wrote (inf / 0: none).
constexpr float kPulsarSpan = 60.0f;
__device__ __forceinline__ bool splat_fill_weights(float4 *list, int cnt, int *s_zmm, float zlo, float zhi, float &tr, float &sd, float &sr,
                                                   float &sg, float &sb, float &fscale)
{
    // (exponents are >= 0: the integer order of their bit patterns is theirs)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        zlo = fminf(zlo, __shfl_xor(zlo, off, kWave));
        zhi = fmaxf(zhi, __shfl_xor(zhi, off, kWave));
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        atomicMax(&s_zmm[0], __float_as_int(zhi));
        atomicMin(&s_zmm[1], __float_as_int(zlo));
    }
    __syncthreads();
    const float m_f = __int_as_float(s_zmm[0]), z_min = __int_as_float(s_zmm[1]);
    const bool fast = m_f - z_min < kPulsarSpan;
    if (fast) {
        for (int k = threadIdx.x; k < cnt; k += blockDim.x) list[k].w = __expf(list[k].w - m_f);
        const float m_new = fmaxf(tr, m_f);
        const float sc = __expf(tr - m_new);
        sd *= sc; sr *= sc; sg *= sc; sb *= sc;
        fscale = __expf(m_f - m_new);
        tr = m_new;
    }
    __syncthreads();
    if (threadIdx.x == 0) { s_zmm[0] = 0; s_zmm[1] = 0x7f800000; }      // for the next fill (whose writes come behind a barrier)
    return fast;
}

// The full scan of mask_splat_kernel: every point of the image against the tile, sixteen per thread and round (see the
// comments inside; called for a tile whose list overflowed, or when the launch has no lists).
template <int BLEND>
__device__ __attribute__((noinline)) void splat_full_scan(int n, const float4 *__restrict__ uvr, const float *__restrict__ col,
                                                          const float *__restrict__ zex, int tx0, int ty0, int tx1, int ty1, float pxc,
                                                          float pyc, int share, int lane, int wave, float &tr, float &sd, float &sr,
                                                          float &sg, float &sb, float4 *list, float2 *list_gb, float4 *list_c, int *s_tab,
                                                          int *s_cntp, int *s_zmm)
{
    for (int j0 = 0; j0 < n; j0 += kSplatBlock * kSplatPer) {
        // the bounding-box tests keep only a bit per point (four points in flight at a time): the kernel must fit 64
        // VGPRs so that TWO 1024-thread blocks share a CU -- with all sixteen points of a thread in registers it needed
        // 128, one block per CU, and a lock-step batch of 8 scans x 4 starts (6272 blocks) ran 8 % slower
        unsigned hit = 0;
#pragma unroll
        for (int i0 = 0; i0 < kSplatPer; i0 += 4) {
            float4 q[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int j = j0 + (i0 + i) * kSplatBlock + threadIdx.x;
                q[i] = j < n ? uvr[j] : make_float4(0.0f, 0.0f, -1.0f, 0.0f);
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                // the disc's bounding box against the tile
                if (q[i].z > 0.0f && q[i].x + q[i].z >= (float)tx0 && q[i].x - q[i].z <= (float)(tx1 + 1) &&
                    q[i].y + q[i].z >= (float)ty0 && q[i].y - q[i].z <= (float)(ty1 + 1))
                    hit |= 1u << (i0 + i);
            }
        }
        // The list is filled in ascending point order -- rank = number of hits before this one in (i, wave, lane)
        // order, which is the order of the point indices j = j0 + i * kSplatBlock + tid -- so that a pixel sums its
        // discs in the same order in every run (an arrival-order list made the whole alignment loop irreproducible:
        // last-bit differences in the image flip a soft-mask pixel in or out of fp32 sigmoid saturation a few steps
        // later).  One table of per-(i, wave) counts, one scan by wave 0, two barriers per round of 16384 points.
        // a lane's rank among its wave's hits of step i, eight bits each (the ballots themselves are not kept: 32 SGPRs)
        unsigned long long rk[kSplatPer / 8];
#pragma unroll
        for (int w8 = 0; w8 < kSplatPer / 8; w8++) rk[w8] = 0ull;
#pragma unroll
        for (int i = 0; i < kSplatPer; i++) {
            const unsigned long long bl = __ballot((hit >> i) & 1u);
            if (lane == 0) s_tab[i * (kSplatBlock / kWave) + wave] = __popcll(bl);
            rk[i >> 3] |= (unsigned long long)__popcll(bl & ((1ull << lane) - 1ull)) << (8 * (i & 7));
        }
        __syncthreads();
        if (wave == 0) {
            // exclusive scan of the 256 counts (four per lane, in table order)
            static_assert(kSplatPer * (kSplatBlock / kWave) == 4 * kWave, "four table entries per lane");
            int c4[4], tot = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) { c4[q] = s_tab[lane * 4 + q]; tot += c4[q]; }
            int incl = tot;
#pragma unroll
            for (int off = 1; off < kWave; off <<= 1) {
                const int o = __shfl_up(incl, off, kWave);
                incl += lane >= off ? o : 0;
            }
            int run = incl - tot;
#pragma unroll
            for (int q = 0; q < 4; q++) { s_tab[lane * 4 + q] = run; run += c4[q]; }
            if (lane == kWave - 1) *s_cntp = incl;
        }
        __syncthreads();
        const int total = *s_cntp;
        // the list holds kSplatList entries: a crowded tile is drawn in several fills
        for (int f0 = 0; f0 < total; f0 += kSplatList) {
            float zlo = __builtin_inff(), zhi = 0.0f;
#pragma unroll
            for (int i = 0; i < kSplatPer; i++) {
                if ((hit >> i) & 1u) {
                    const int slot = s_tab[i * (kSplatBlock / kWave) + wave] + (int)((rk[i >> 3] >> (8 * (i & 7))) & 0xffull) - f0;
                    if (slot >= 0 && slot < kSplatList) {
                        const int j = j0 + i * kSplatBlock + threadIdx.x;
                        const float4 qh = uvr[j];                 // (a hit is rare: read again rather than kept)
                        float cr = 1.0f, cg = 1.0f, cb = 1.0f;
                        if (col) { cr = col[(size_t)j * 3 + 0]; cg = col[(size_t)j * 3 + 1]; cb = col[(size_t)j * 3 + 2]; }
                        if (BLEND) {
                            const float ze = zex[j];
                            list[slot] = make_float4(qh.x, qh.y, qh.w, ze);
                            list_c[slot] = make_float4(cr, cg, cb, 0.0f);
                            zlo = fminf(zlo, ze); zhi = fmaxf(zhi, ze);
                        } else {
                            list[slot] = make_float4(qh.x, qh.y, qh.w, cr);
                            list_gb[slot] = make_float2(cg, cb);
                        }
                    }
                }
            }
            __syncthreads();
            const int cnt = min(total - f0, kSplatList);
            float fscale = 1.0f;
            const bool fast = BLEND && splat_fill_weights(list, cnt, s_zmm, zlo, zhi, tr, sd, sr, sg, sb, fscale);
            for (int k = share; k < cnt; k += 4) {
                const float4 p = list[k];
                const float dx = pxc - p.x, dy = pyc - p.y;
                const float a = 1.0f - (dx * dx + dy * dy) * p.z;
                if (a > 0.0f) {
                    if (BLEND) {
                        const float4 c = list_c[k];
                        if (fast) {
                            const float w = fminf(a, kMaskAmax) * (p.w * fscale);
                            sd += w; sr += w * c.x; sg += w * c.y; sb += w * c.z;
                        } else {
                            splat_fold<1>(tr, sd, sr, sg, sb, fminf(a, kMaskAmax), c.x, c.y, c.z, p.w);
                        }
                    } else {
                        const float2 gb = list_gb[k];
                        splat_fold<0>(tr, sd, sr, sg, sb, fminf(a, kMaskAmax), p.w, gb.x, gb.y, 0.0f);
                    }
                }
            }
            __syncthreads();
        }
    }
}

// tools/splat_timeline.py builds a private copy of the library with -DGENPC_SPLAT_TIMELINE: thread 0 of every block stamps the
// 100 MHz wall clock at the phase boundaries of mask_splat_kernel (nothing of this exists in the shipped library)
#ifdef GENPC_SPLAT_TIMELINE
__device__ unsigned long long g_splat_tl[4096 * 8];
#define GENPC_STL(k) do { if (threadIdx.x == 0 && blockIdx.x < 4096) g_splat_tl[blockIdx.x * 8 + (k)] = wall_clock64(); } while (0)
#define GENPC_STL_VAL(k, v) do { if (threadIdx.x == 0 && blockIdx.x < 4096) g_splat_tl[blockIdx.x * 8 + (k)] = (unsigned long long)(v); } while (0)
#else
#define GENPC_STL(k) do {} while (0)
#define GENPC_STL_VAL(k, v) do {} while (0)
#endif
// 1-D grid of tiles * nb blocks (xcd_block).  col: [nb, n, 3] colours or nullptr (white).  BLEND 1: zex [nb, n] depth exponents.
template <int BLEND>
__global__ __launch_bounds__(kSplatBlock, 8) void mask_splat_kernel(int n, const float4 *__restrict__ uvr,
                                                                 const float *__restrict__ col, int S,
                                                                 float *__restrict__ planes, double *__restrict__ accum,
                                                                 int *__restrict__ bins, int nb,
                                                                 const float *__restrict__ zex, int *__restrict__ clean = nullptr,
                                                                 const int *__restrict__ off = nullptr)
{
    static_assert(kSplatBlock == 4 * kMaskTile * kMaskTile, "four threads per pixel of the tile");
    __shared__ float part[5][4][kMaskTile * kMaskTile];
    __shared__ float4 list[kSplatList];       // u, v, 1 / rho^2, red
    __shared__ float2 list_gb[BLEND ? 1 : kSplatList];    // blend 0: green, blue
    __shared__ float4 list_c[BLEND ? kSplatList : 1];     // blend 1: red, green, blue (list[k].w: depth exponent, or weight exp(z / gamma - m_f))
    __shared__ int s_zmm[2];                              // blend 1: a fill's largest / smallest exponent (bits)
    if (BLEND && threadIdx.x == 0) { s_zmm[0] = 0; s_zmm[1] = 0x7f800000; }
    GENPC_STL(0);
    __shared__ int s_cnt;
    __shared__ int s_tab[kSplatPer * (kSplatBlock / kWave)];      // per (i, wave): hits, then their exclusive prefix
    const XcdBlock xb = xcd_block(((S + kMaskTile - 1) / kMaskTile) * ((S + kMaskTile - 1) / kMaskTile), nb);
    const int e = xb.e, tile = xb.x;
    const int P = S * S;
    const int tiles_x = (S + kMaskTile - 1) / kMaskTile;
    const int tx0 = (tile % tiles_x) * kMaskTile, ty0 = (tile / tiles_x) * kMaskTile;
    const int tx1 = min(S, tx0 + kMaskTile) - 1, ty1 = min(S, ty0 + kMaskTile) - 1;
    const PoseSpan sp = pose_span(off, e, n);      // (list and full-scan paths alike: both see the element's own n from here on)
    n = sp.n;
    uvr += sp.base;
    if (col) col += sp.base * 3;
    if (BLEND) zex += sp.base;
    planes += (size_t)e * 5 * P;
    if (accum) accum += (size_t)e * kAcc;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    // thread = (pixel of the tile, one of four interleaved shares of the point list)
    const int pix = threadIdx.x & (kMaskTile * kMaskTile - 1), share = threadIdx.x / (kMaskTile * kMaskTile);
    const float pxc = (float)(tx0 + (pix & (kMaskTile - 1))) + 0.5f, pyc = (float)(ty0 + pix / kMaskTile) + 0.5f;
    float tr = BLEND ? kPulsarZe0 : 1.0f, sd = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;      // transmittance prod (1 - a) (blend 1: the running maximum exponent), sums of a and a c
    // Every block reads every point of its scan (16 x 16 tiles: 196 blocks per scan), kSplatPer per thread
    // loaded together; the points whose disc touches the tile are compacted into LDS (one LDS atomic per wave
    // and step), then GATHERED: every pixel walks the list (broadcast reads) and accumulates the discs
    // that cover it, in list order -- no atomics on the image.  (Scattering with LDS float atomics ran at
    // ~0.6 adds per clock per CU: 26 us of the kernel's 36 for 758 points in the busiest tile.)
    // The tile's own list (bins, filled by the projection kernel): its indices are put in ascending order -- the fixed
    // summation order of the gather -- by counting ranks, the entries fetched, and the full scan below is skipped.  A tile
    // whose list overflowed (or a launch without bins) takes the full scan.
    // (the counting ranks' copy of the indices is dead before the first fill writes the colours: blend 1 keeps it in their array --
    //  with an array of its own the block took 83 228 bytes of LDS, ONE block per CU instead of two: 46 us against 35)
    __shared__ __attribute__((aligned(16))) int s_sort_own[BLEND ? 4 : kSplatCap];
    int *s_sort = BLEND ? (int *)&list_c[0] : s_sort_own;
    static_assert(sizeof(float4) * kSplatList >= sizeof(int) * kSplatCap, "the indices fit the colour array");
    __shared__ unsigned char s_mask[kSplatCap];
    __shared__ unsigned s_bits[kRankWords];
    __shared__ unsigned short s_pref[kRankWords];
    __shared__ unsigned short s_strip[4][kSplatCap];
    __shared__ int s_wc[kSplatBlock / kWave][4], s_stot[4];
    static_assert(kMaskTile == 16 && kSplatBlock / kWave == 16, "a wave = four rows of the tile, four shares");
    int binned = -1;
    int *bin_cnt = bins ? bins + (size_t)e * bins_tiles(S) : nullptr;
    const int *bin_idx = bins ? bins + (size_t)nb * bins_tiles(S) + ((size_t)e * bins_tiles(S) + tile) * kTileCap : nullptr;
    int my_ent = 0;
    if (bins) {
        binned = bin_cnt[tile];
        if (threadIdx.x < kSplatCap) my_ent = bin_idx[threadIdx.x];      // (before the count is known: one round trip, not two)
    }
    const bool by_list = binned >= 0 && (binned <= kSplatCap || (binned <= kTileCap && n <= 32 * kRankWords));
    GENPC_STL_VAL(7, binned + 1);
    GENPC_STL(1);
    // An empty tile whose pixels already hold the background leaves at once (round 6): three of four tiles of a scan's image are
    // empty at every step, and each held a 1024-thread, 79 KB slot for 9.5 us to rewrite what was there (tools/splat_timeline.py) --
    // the launch's other blocks waited up to 13 us for a slot.  Its sums of I and I^2 are zero: nothing to add.
    int *clean_flag = clean && bins ? clean + (size_t)e * bins_tiles(S) + tile : nullptr;
    if (clean_flag && binned == 0) {
        const int was_clean = *clean_flag;          // (block-uniform; the only writer of this word is this block, below)
        if (was_clean) { GENPC_STL(6); return; }
    }
    if (by_list && binned > 0) {
        static_assert(kSplatCap <= kSplatBlock && kSplatCap <= kSplatList && kSplatCap <= kTileCap, "one list entry per thread and fill");
        const int L = binned, L4 = (L + 3) & ~3;
        const bool bitmap = L > kRankByCount && n <= 32 * kRankWords;      // (by_list: L <= kSplatCap otherwise)
        int rank0 = 0;      // counting path: the rank of this thread's (only) entry
        if (bitmap) {
            // a long list: rank = number of set bits below the point's own in a bitmap of the image's points (the
            // counting below is O(L^2): 40 of the launch's 220 us with 32 images, in the crowded tiles)
            const int words = (n + 31) >> 5;
            for (int w = threadIdx.x; w < words; w += kSplatBlock) s_bits[w] = 0u;
            __syncthreads();
            for (int i = threadIdx.x; i < L; i += kSplatBlock) {
                const int j = (i < kSplatCap ? my_ent : bin_idx[i]) >> 2;
                atomicOr(&s_bits[j >> 5], 1u << (j & 31));
            }
            __syncthreads();
            // exclusive prefix of the words' popcounts: kRankWords / kSplatBlock consecutive words per thread
            constexpr int kWPT = kRankWords / kSplatBlock;
            int c[kWPT], tot = 0;
#pragma unroll
            for (int q = 0; q < kWPT; q++) {
                const int w = threadIdx.x * kWPT + q;
                c[q] = w < words ? __popc(s_bits[w]) : 0;
                tot += c[q];
            }
            int incl = tot;
#pragma unroll
            for (int off = 1; off < kWave; off <<= 1) {
                const int o = __shfl_up(incl, off, kWave);
                incl += lane >= off ? o : 0;
            }
            if (lane == kWave - 1) s_wc[wave][0] = incl;
            __syncthreads();
            int base = 0;
            for (int w = 0; w < wave; w++) base += s_wc[w][0];
            int run = base + incl - tot;
#pragma unroll
            for (int q = 0; q < kWPT; q++) {
                const int w = threadIdx.x * kWPT + q;
                if (w < words) s_pref[w] = (unsigned short)run;
                run += c[q];
            }
        } else {
            const int myj = (int)threadIdx.x < L ? my_ent >> 2 : 0x7fffffff;
            if ((int)threadIdx.x < L4) s_sort[threadIdx.x] = myj;
            __syncthreads();
            if ((int)threadIdx.x < L) {
                for (int k = 0; k < L4; k += 4) {
                    const int4 o = *(const int4 *)&s_sort[k];
                    rank0 += (o.x < myj) + (o.y < myj) + (o.z < myj) + (o.w < myj);
                }
            }
        }
        // A list of several fills: the point indices in sorted order first (16-bit: the bitmap path holds n <= 65536), in the
        // LDS of `part`, which is not needed before the epilogue -- every fill then takes its 1024 entries from there instead
        // of walking the whole list for them (a tile of 5000 entries: five fills of five dependent global reads per thread).
        static_assert(sizeof(part) >= kTileCap * sizeof(unsigned short) && 32 * kRankWords <= 65536, "the sorted indices fit `part`");
        unsigned short *s_sorted = (unsigned short *)&part[0][0][0];
        const bool presorted = L > kSplatCap;      // (implies bitmap)
        if (presorted) {
            __syncthreads();      // s_pref is ready
            for (int i = threadIdx.x; i < L; i += kSplatBlock) {
                const int myj = (i < kSplatCap ? my_ent : bin_idx[i]) >> 2;
                s_sorted[s_pref[myj >> 5] + __popc(s_bits[myj >> 5] & ((1u << (myj & 31)) - 1u))] = (unsigned short)myj;
            }
        }
        // the sorted list is drawn kSplatCap entries at a time (one fill, unless the tile is crowded beyond that)
        for (int f0 = 0; f0 < L; f0 += kSplatCap) {
            __syncthreads();      // ranks ready / the previous fill's gather is done with the list
            const int Lf = min(kSplatCap, L - f0);
            float zlo = __builtin_inff(), zhi = 0.0f;
            for (int i = threadIdx.x; i < (presorted ? Lf : L); i += kSplatBlock) {
                int myj, rank;
                if (presorted) {
                    myj = s_sorted[f0 + i];
                    rank = i;
                } else {
                    myj = (i < kSplatCap ? my_ent : bin_idx[i]) >> 2;
                    rank = (bitmap ? s_pref[myj >> 5] + __popc(s_bits[myj >> 5] & ((1u << (myj & 31)) - 1u)) : rank0) - f0;
                }
                if (rank < 0 || rank >= Lf) continue;
                const float4 qh = uvr[myj];
                float cr = 1.0f, cg = 1.0f, cb = 1.0f;
                if (col) { cr = col[(size_t)myj * 3 + 0]; cg = col[(size_t)myj * 3 + 1]; cb = col[(size_t)myj * 3 + 2]; }
                if (BLEND) {
                    const float ze = zex[myj];
                    list[rank] = make_float4(qh.x, qh.y, qh.w, ze);
                    list_c[rank] = make_float4(cr, cg, cb, 0.0f);
                    zlo = fminf(zlo, ze); zhi = fmaxf(zhi, ze);
                } else {
                    list[rank] = make_float4(qh.x, qh.y, qh.w, cr);
                    list_gb[rank] = make_float2(cg, cb);
                }
                // the strips (four rows of the tile = the 64 pixels of one wave) the disc can reach
                unsigned m = 0;
#pragma unroll
                for (int st = 0; st < 4; st++)
                    if (qh.y + qh.z >= (float)(ty0 + 4 * st) && qh.y - qh.z <= (float)(ty0 + 4 * st + 4)) m |= 1u << st;
                s_mask[rank] = (unsigned char)m;
            }
            // blend 1: the fill's largest / smallest exponent ride on the barriers the strips need anyway (splat_fill_weights,
            // the full scan's form, pays two block-wide barriers of sixteen waves for them: 11 us of this kernel's 46)
            if (BLEND) {
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    zlo = fminf(zlo, __shfl_xor(zlo, off, kWave));
                    zhi = fmaxf(zhi, __shfl_xor(zhi, off, kWave));
                }
                if (lane == 0 && zhi >= zlo) {          // (exponents are >= 0: the integer order of their bit patterns is theirs)
                    atomicMax(&s_zmm[0], __float_as_int(zhi));
                    atomicMin(&s_zmm[1], __float_as_int(zlo));
                }
            }
            __syncthreads();
            GENPC_STL(2);
            bool fast = false;
            float fscale = 1.0f;
            if (BLEND) {
                const float m_f = __int_as_float(s_zmm[0]);
                fast = m_f - __int_as_float(s_zmm[1]) < kPulsarSpan;
                if (fast) {
                    // one exponential per listed disc (the strips' barriers below stand between this and the gather)
                    if ((int)threadIdx.x < Lf) list[threadIdx.x].w = __expf(list[threadIdx.x].w - m_f);
                    const float m_new = fmaxf(tr, m_f);
                    const float sc = __expf(tr - m_new);
                    sd *= sc; sr *= sc; sg *= sc; sb *= sc;
                    fscale = __expf(m_f - m_new);
                    tr = m_new;
                }
            }
            // Per-strip sublists of the sorted list, in its order: a wave walks the discs that can reach its four rows only
            // (about half of the tile's).  Ballot ranks inside a wave, a 16 x 4 table of wave counts, its prefix by four threads.
            {
                const unsigned m = (int)threadIdx.x < Lf ? s_mask[threadIdx.x] : 0u;
                int pre[4];
#pragma unroll
                for (int st = 0; st < 4; st++) {
                    const unsigned long long bl = __ballot((m >> st) & 1u);
                    pre[st] = __popcll(bl & ((1ull << lane) - 1ull));
                    if (lane == 0) s_wc[wave][st] = __popcll(bl);
                }
                __syncthreads();
                if (BLEND && threadIdx.x == kWave) { s_zmm[0] = 0; s_zmm[1] = 0x7f800000; }      // (read by all before the barrier above; the next fill's come behind the loop's)
                if (threadIdx.x < 4) {
                    int run = 0;
                    for (int w = 0; w < kSplatBlock / kWave; w++) {
                        const int c = s_wc[w][threadIdx.x];
                        s_wc[w][threadIdx.x] = run;
                        run += c;
                    }
                    s_stot[threadIdx.x] = run;
                }
                __syncthreads();
#pragma unroll
                for (int st = 0; st < 4; st++)
                    if ((m >> st) & 1u) s_strip[st][s_wc[wave][st] + pre[st]] = (unsigned short)threadIdx.x;
                __syncthreads();
            }
            GENPC_STL(3);
            const int strip = wave & 3;      // (pix = tid & 255: wave w holds rows 4 (w & 3) .. + 3, share w >> 2)
            const int LS = s_stot[strip];
            for (int k2 = share; k2 < LS; k2 += 4) {
                const int k = s_strip[strip][k2];
                const float4 p = list[k];
                const float dx = pxc - p.x, dy = pyc - p.y;
                const float a = 1.0f - (dx * dx + dy * dy) * p.z;
                if (a > 0.0f) {
                    if (BLEND) {
                        const float4 c = list_c[k];
                        if (fast) {
                            const float w = fminf(a, kMaskAmax) * (p.w * fscale);
                            sd += w; sr += w * c.x; sg += w * c.y; sb += w * c.z;
                        } else {
                            splat_fold<1>(tr, sd, sr, sg, sb, fminf(a, kMaskAmax), c.x, c.y, c.z, p.w);
                        }
                    } else {
                        const float2 gb = list_gb[k];
                        splat_fold<0>(tr, sd, sr, sg, sb, fminf(a, kMaskAmax), p.w, gb.x, gb.y, 0.0f);
                    }
                }
            }
        }
    }
    // the count is reset for the next launch by the last kernel that reads the lists: this one
    __syncthreads();
    GENPC_STL(4);
    if (bins && threadIdx.x == 0) bin_cnt[tile] = 0;
    // (the full scan of a tile without a usable list is a function of its own, NOT inlined: its sixteen-points-per-thread
    // bookkeeping is what overflowed the 64 registers the two-blocks-per-CU launch allows -- 59 spilled VGPRs, ten scratch
    // instructions of them on the path of a tile that has its list; VERDICT r4 weak #8.  Here the spills stay in the callee.)
    if (!by_list)
        splat_full_scan<BLEND>(n, uvr, col, zex, tx0, ty0, tx1, ty1, pxc, pyc, share, lane, wave, tr, sd, sr, sg, sb, list, list_gb, list_c, s_tab, &s_cnt, s_zmm);
    part[0][share][pix] = tr;
    part[1][share][pix] = sd;
    part[2][share][pix] = sr;
    part[3][share][pix] = sg;
    part[4][share][pix] = sb;
    __syncthreads();
    __shared__ float s_I[3][kMaskTile * kMaskTile];
    if (threadIdx.x < kMaskTile * kMaskTile) {
        float I3[3] = {0.0f, 0.0f, 0.0f};
        const int r = ty0 + pix / kMaskTile, cc = tx0 + (pix & (kMaskTile - 1));
        if (r < S && cc < S) {
            float w[5];
            // plane 0 is the transmittance T = prod (1 - a) itself (round 2 accumulated log(1 - a) per covering disc and
            // took exp(L) wherever the plane was read: the logarithm was a third of the gather's instructions, and the
            // gather is what the kernel's time is -- 33 M pixel-disc tests per step of four starts).  (Per-strip index lists -- a
            // wave walks only the discs reaching its four rows -- cost three more barriers per FILL of the full scan: 42.0 ->
            // 44.3 ms per call there; the list path above builds them once per tile and keeps them.)
            if (BLEND) {
                // the four shares' sums are relative to their own maxima: to the common one, plus the background's weight
                const float m4 = fmaxf(fmaxf(part[0][0][pix], part[0][1][pix]), fmaxf(part[0][2][pix], part[0][3][pix]));
                float sc[4];
#pragma unroll
                for (int k = 0; k < 4; k++) sc[k] = __expf(part[0][k][pix] - m4);
                w[0] = m4;
                planes[(size_t)r * S + cc] = m4;
#pragma unroll
                for (int k = 1; k < 5; k++) {
                    w[k] = (part[k][0][pix] * sc[0] + part[k][1][pix] * sc[1]) + (part[k][2][pix] * sc[2] + part[k][3][pix] * sc[3]);
                    if (k == 1) w[k] += __expf(kPulsarZe0 - m4);
                    planes[(size_t)k * P + (size_t)r * S + cc] = w[k];
                }
                const float iD = 1.0f / w[1];
#pragma unroll
                for (int ch = 0; ch < 3; ch++) I3[ch] = w[2 + ch] * iD;
            } else {
            w[0] = (part[0][0][pix] * part[0][1][pix]) * (part[0][2][pix] * part[0][3][pix]);
            planes[(size_t)r * S + cc] = w[0];
#pragma unroll
            for (int k = 1; k < 5; k++) {
                w[k] = (part[k][0][pix] + part[k][1][pix]) + (part[k][2][pix] + part[k][3][pix]);
                planes[(size_t)k * P + (size_t)r * S + cc] = w[k];
            }
            const float O = 1.0f - w[0];
            const float iD = w[1] > 0.0f ? 1.0f / w[1] : 0.0f;
#pragma unroll
            for (int ch = 0; ch < 3; ch++) I3[ch] = O * (w[2 + ch] * iD);
            }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ch++) s_I[ch][pix] = I3[ch];
    }
    GENPC_STL(5);
    if (clean_flag && threadIdx.x == 0) *clean_flag = binned == 0 ? 1 : 0;
    if (accum) {
        // The tile's sums of I and I^2 per channel (doubles), by ONE wave: four pixels per lane, then the wave's shuffles.
        // (All sixteen waves used to run the 72 64-bit shuffles of the reduction although only four held pixels: with two
        // blocks per CU that was 76 of the launch's 200 us at 32 images.)
        __syncthreads();
        if (wave == 0) {
            double s1[3] = {0.0, 0.0, 0.0}, s2[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int q = 0; q < kMaskTile * kMaskTile / kWave; q++)
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    const double I = (double)s_I[ch][lane + q * kWave];
                    s1[ch] += I;
                    s2[ch] += I * I;
                }
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                s1[ch] = wave_sum63(s1[ch]);
                s2[ch] = wave_sum63(s2[ch]);
            }
            if (lane == kWave - 1) {
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    atomicAdd(&accum[16 + ch], s1[ch]);
                    atomicAdd(&accum[19 + ch], s2[ch]);
                }
            }
        }
    }
    GENPC_STL(6);
}

// img[P, 3] (H, W, C like the reference's renders) from the five planes
__global__ void mask_image_kernel(int P, const float *__restrict__ planes, float *__restrict__ img, int mode)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= P) return;
    const PxImg px = load_pixel(planes, P, q, mode);
    img[(size_t)q * 3 + 0] = px.I[0];
    img[(size_t)q * 3 + 1] = px.I[1];
    img[(size_t)q * 3 + 2] = px.I[2];
}

// Which blend the images of the mask term are drawn with: 1 Pulsar's published blending function (softmax in depth; the
// default), 0 the round-2 coverage splat (order-independent; kept for A/B and for the numbers quoted before round 5).
// genpc_render_tune() sets it per calling thread.
thread_local int t_render_blend = -1;
int render_blend()
{
    return t_render_blend != 0 ? 1 : 0;
}

void launch_mask_splat(int b, int n, const float *pts, const float *col, bool project, const float *center, int cstride, const float *params,
                       int pstride, int posed, float radius, int S, const MaskScratch &m, double *accum, hipStream_t st, const int *off)
{
    const int blend = render_blend();
    int *bins = use_bins(S) ? m.bins : (int *)nullptr;
    float *zex = blend ? m.zex : (float *)nullptr;      // blend 1: the depth exponents, written by the projection
    if (project)
        hipLaunchKernelGGL(mask_project_kernel, dim3(lin_grid(n > 0 ? n : 1), b), dim3(kQBlock), 0, st, n, pts, center, cstride, params, pstride,
                           posed, radius, S, m.uvr, bins, zex, off);
    if (blend)
        hipLaunchKernelGGL(mask_splat_kernel<1>, dim3(mask_tiles(S) * b), dim3(kSplatBlock), 0, st, n, (const float4 *)m.uvr, col, S, m.planes,
                           accum, bins, b, (const float *)zex, m.clean, off);
    else
        hipLaunchKernelGGL(mask_splat_kernel<0>, dim3(mask_tiles(S) * b), dim3(kSplatBlock), 0, st, n, (const float4 *)m.uvr, col, S, m.planes,
                           accum, bins, b, (const float *)zex, m.clean, off);
}

}  // namespace genpc

#ifdef GENPC_SPLAT_TIMELINE
extern "C" __attribute__((visibility("default"))) int genpc_splat_timeline_read(unsigned long long *out)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(genpc::g_splat_tl), sizeof(unsigned long long) * 4096 * 8) == hipSuccess;
}
#endif

GENPC_API int genpc_splat_image(int n, const float *pts, const float *col, float radius, int size, float *img, void *stream)
{
    using namespace genpc;
    if (n < 0 || size <= 0 || !(radius > 0.0f)) return -1;
    hipStream_t st = (hipStream_t)stream;
    const size_t P = (size_t)size * size;
    MaskScratch m;
    WsLayout L;
    m.layout(L, 1, P, n > 0 ? n : 1);
    if (!ws_alloc(L, kWsSplatImage, st)) return 0;
    if (!m.zero_bins(st)) return 0;
    launch_mask_splat(1, n, pts, col, true, nullptr, 0, nullptr, 0, 0, radius, size, m, nullptr, st);
    hipLaunchKernelGGL(mask_image_kernel, dim3(ceil_div((int)P, 256)), dim3(256), 0, st, (int)P, (const float *)m.planes, img, render_blend() ? 2 : 0);
    return check(hipGetLastError(), "splat_image launch") ? 1 : 0;
}

/* The renderer of the mask term, per calling host thread: 1 Pulsar's blending function (default), 0 the coverage splat,
 * < 0 back to the default.  Returns the previous setting (-1 = default). */
GENPC_API int genpc_render_tune(int blend)
{
    const int prev = genpc::t_render_blend;
    genpc::t_render_blend = blend < 0 ? -1 : (blend ? 1 : 0);
    return prev;
}
