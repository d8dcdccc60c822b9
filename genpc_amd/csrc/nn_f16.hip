// nn_f16.hip -- nearest-neighbour filter with ONE v_mfma_f32_32x32x16_f16 per 32x32 tile.
//
// Filter-and-prove scheme (the finish half is nn_finish.hip).  A split-bf16 variant would
// need two chained instructions per tile (three 8-bit pieces per operand, 27 products) and
// was retired in round 3.  An f16 piece carries 11 bits, so two pieces v = h + l (h = RN16(v), l = RN16(v - h), residual
// <= 2^-22 |v|) and all four products per coordinate fit the K = 16 of a single
// instruction:
//     lanes  0..31 (k 0..7):   A = [xh,xh,xl,xl, yh,yh,yl,yl]   B = [qxh,qxl,qxh,qxl, qyh,qyl,qyh,qyl]
//     lanes 32..63 (k 8..15):  A = [zh,zh,zl,zl, Th,Tl,0,0]     B = [qzh,qzl,qzh,qzl, 2^8,2^8,0,0]
// with x.. the pieces of -2 s x', q.. of s q', T of s^2 |t'|^2 2^-8.  f16 has a narrow
// exponent range, so each block scales by a power of two s (exact) that puts the largest
// centred coordinate of ITS queries and ITS target slice in [2^10, 2^11): products stay
// below 2^23, |t'|^2 s^2 2^-8 below 3 x 2^14, small coordinates may reach f16 subnormals,
// which the instruction does not flush (tools/ubench_mfma_f16.hip) -- their absolute
// error, <= 2^-25 in scaled units, is far below the bound.  The list values s^2 (|t'|^2 -
// 2 q'.t') are unscaled (two exact multiplications) when the lists are published.
//
// Error bound, u = 2^-24, T = max |t'|: residuals 4u per operand -> 16u |q'|T on
// -2 q'.t' and 4u T^2 on |t'|^2; the instruction's summation, measured at <= 3.1 u
// sum|terms| (adversarial cancellation, profiles/r01_ubench_mfma_f16.txt), budgeted at
// 6.5u (2|q'|T + T^2); three fp32 roundings each in |t'|^2 and |q'|^2; one unit on T^2
// for subnormal pieces:  E1 = u (30 |q'| T + 15 T^2 + 3 |q'|^2).
#include "nn.h"
#include <hip/hip_ext.h>
#include "../../include/genpc_hip.h"

#include <stdlib.h>

namespace genpc {

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));

// tools/nn_timeline.py builds a private copy of the library with -DGENPC_NN_TIMELINE: thread 0 of every block stamps the
// shader clock at the phase boundaries of nn_f16_kernel (nothing of this exists in the shipped library)
#ifdef GENPC_NN_TIMELINE
// (rows of kTimelineRow words: 0-5 the phase boundaries, 6-7 the wall clock at a block's start and end, 8 the moment before the
// block's first vector load is issued -- everything in front of it is kernel arguments and the block decode; 9-11 the partner
// wave: lane 0 of wave 4, which shares wave 0's SIMD in the wide form, at its MFMA loop's start, its end and "lists published" --
// word 4 is wave 0's loop end, and the two waves of a block read the same counter)
constexpr int kTimelineRow = 16;
__device__ unsigned long long g_timeline[4096 * kTimelineRow];
#define GENPC_TL(k) do { if (threadIdx.x == 0 && blockIdx.x < 4096) { g_timeline[blockIdx.x * kTimelineRow + (k)] = __builtin_readcyclecounter(); \
    if ((k) == 0) g_timeline[blockIdx.x * kTimelineRow + 6] = wall_clock64(); if ((k) == 5) g_timeline[blockIdx.x * kTimelineRow + 7] = wall_clock64(); } } while (0)
#define GENPC_TL_PARTNER(k) do { if (WV == 8 && threadIdx.x == 4 * kWave && blockIdx.x < 4096) g_timeline[blockIdx.x * kTimelineRow + (k)] = __builtin_readcyclecounter(); } while (0)
#else
#define GENPC_TL(k) do {} while (0)
#define GENPC_TL_PARTNER(k) do {} while (0)
#endif
constexpr double kQTh = 30.0, kTTh = 15.0;

__device__ __forceinline__ unsigned f16_bits(float v) { return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)v); }

// v = h + l in f16 (v already scaled into range); returns h | l << 16
__device__ __forceinline__ unsigned split2(float v)
{
    const _Float16 h = (_Float16)v;
    const _Float16 l = (_Float16)(v - (float)h);
    return (unsigned)__builtin_bit_cast(unsigned short, h) | ((unsigned)__builtin_bit_cast(unsigned short, l) << 16);
}

__device__ __forceinline__ unsigned dup_lo(unsigned v) { return __builtin_amdgcn_perm(v, v, 0x01000100u); }
__device__ __forceinline__ unsigned dup_hi(unsigned v) { return __builtin_amdgcn_perm(v, v, 0x03020302u); }

// largest power of two s with s * m < 2^11 (m > 0 finite), 1 otherwise
__device__ __forceinline__ float scale_for(float m)
{
    if (!(m > 0.0f) || !(m < __builtin_inff())) return 1.0f;
    const int e = __builtin_amdgcn_frexp_expf(m);       // m = f * 2^e, f in [0.5, 1)
    return __builtin_ldexpf(1.0f, 11 - e);
}

// One block = one (direction, target slice, batch, 128*Q-query block) unit; wave w owns Q
// tiles of 32 queries.  U = target tiles per bookkeeping unit, NL = candidate lists per lane.
// W = waves per SIMD the register budget is held to (Q = 4: 182-202 VGPRs natural -> 2 waves; W = 3
// caps at 168 with ~50-150 B of scratch: +1 us on a single-round launch, -4 % over many rounds)
// The lists go to nn_finish_kernel (nn_finish.hip), a second launch.  (Round 2 also carried a fused form -- the last
// slice block to arrive for a query block ran the finish step itself: 13x16384^2 313 -> 296 us but 1x16384^2
// 36 -> 59, and a cliff on scan-like clouds whose 512-query blocks overflow the block's work list -- and a
// Morton-sorted mode that culled whole (query block, slice) pairs: 336 -> 532 us on the 13 scans.  Both lost on
// the inputs that matter and were removed in round 3; DESIGN.md section 4.1 keeps the measurements.)
template <int Q, int U, int NL, int W, int HT, int WV>
__global__ __launch_bounds__(WV * kWave, W) void nn_f16_kernel(NNArgs a)
{
    // WV waves per block (4, or 8 for the wide single-round form: 1024 queries share one staged slice)
    constexpr int kThreads = WV * kWave;
    // Hazard: the accumulators are consumed by inline-asm v_min3, which the compiler's hazard
    // recognizer does not pad (an 8-pass MFMA result needs 11 wait states before a VALU
    // read).  The pipeline supplies them by construction when Q >= 2: between the MFMA that
    // writes acc[r] and the first read of acc[r] lie the other query tiles' slots, each 8
    // v_min3 + one MFMA (Q = 2: plus an explicit s_nop).  With Q = 1 the read follows at
    // once -- measured: 25 % wrong minima -- so that case is not instantiated.
    static_assert(Q >= 2, "one accumulator chain per wave violates the MFMA -> VALU wait states");
    constexpr int kC = 32 * U;
    constexpr int kRows = HT + 64;              // + two spare tiles: the pipeline fetches two tiles ahead
    __shared__ uint4 plane[2][kRows];
    __shared__ float s_red[WV];
    GENPC_TL(0);
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int half = lane >> 5, col = lane & 31;
    // every kernel argument the block uses, in one round (nn.h, above NN_ARG); the decode divides by multiplying (nn_decode.h)
    int ndir = a.ndir, nbatch = a.b, slice_len = a.slice_len, debug = a.debug;
    NNDiv by_b = a.by_b;
    NN_ARG(int, begin, block_begin); NN_ARG(int, qblocks, qblocks); NN_ARG(NNDiv, by_q, by_qblocks);
    NN_ARG(int, nq, nq); NN_ARG(int, nt, nt); NN_ARG(int, slices, slices); NN_ARG(int, dupsh, dup_shared);
    NN_ARG_PTR(const float, q, q); NN_ARG_PTR(const float, t, t); NN_ARG_PTR(const unsigned, dup, dupmask);
    NN_ARG_PTR(float, tmaxp, tmaxp); NN_ARG_PTR(unsigned long long, part, part);
    asm volatile("" : "+s"(ndir), "+s"(nbatch), "+s"(slice_len), "+s"(debug), "+s"(by_b.mul), "+s"(by_b.shift), NN_HELD(begin), NN_HELD(qblocks),
                 "+s"(by_q_0.mul), "+s"(by_q_0.shift), "+s"(by_q_1.mul), "+s"(by_q_1.shift), NN_HELD(nq), NN_HELD(nt), NN_HELD(slices), NN_HELD(dupsh),
                 NN_HELD(q), NN_HELD(t), NN_HELD(dup), NN_HELD(tmaxp), NN_HELD(part));
    const int d = (ndir > 1 && (int)blockIdx.x >= begin_1) ? 1 : 0;
    const int qblocks = NN_OF_DIR(qblocks), nq = NN_OF_DIR(nq), nt = NN_OF_DIR(nt), slices = NN_OF_DIR(slices), dup_shared = NN_OF_DIR(dupsh);
    const float *const t_dir = (const float *)NN_OF_DIR(t);
    const float *const t_dir0 = (const float *)t_0;
    const int nt_dir0 = nt_0;
    const unsigned *const dup_dir = (const unsigned *)NN_OF_DIR(dup);
    float *const tmaxp_dir = (float *)NN_OF_DIR(tmaxp);
    unsigned long long *const part_dir = (unsigned long long *)NN_OF_DIR(part);
    const NNBlockId id = nn_decode_block((int)blockIdx.x - NN_OF_DIR(begin), qblocks, NNDiv{NN_OF_DIR(by_q).mul, NN_OF_DIR(by_q).shift}, nbatch, by_b);
    const int qb = id.qb, batch = id.batch, slice = id.slice;

    const float *__restrict__ T = t_dir + (size_t)batch * nt * 3;
    // both clouds are centred on the first point of the direction-0 target cloud
    const auto cptr = NN_CONST(t_dir0 + (size_t)batch * nt_dir0 * 3);
    const float cx = cptr[0], cy = cptr[1], cz = cptr[2];

    const int k_begin = slice * slice_len;
    int k_end = k_begin + slice_len;
    if (k_end > nt) k_end = nt;

    // Prologue loads: this lane's queries and -- when the slice fits one LDS tile -- the block's whole slice are
    // requested back to back, before any of the values is used: one memory round trip behind the kernel boundary
    // (with the loads where each value was first needed, the Q query tiles and the slice made Q + 1 round trips in a
    // row, and every word of the duplicate mask one more -- DESIGN_NOTEBOOK.md, "prologue loads").
    // raw coordinates of this lane's queries: lanes < 32 carry x and y, lanes >= 32 z (every lane loads the whole point and
    // drops what it does not carry: a load that every lane issues needs no branch, and a branch would hold its own wait)
    // Addresses: batch element, query block and slice are the block's, so each cloud has a scalar base and a lane adds a
    // 32-bit offset to it (nn_load_point); a query tile is one 12-byte load per lane.
    float raw0[Q], raw1[Q];
    const int qfirst = qb * (WV * 32 * Q);         // the block's first query: below nq
    const int q0 = qfirst + wave * (32 * Q) + col;
    const auto q_base = (NN_GLOBAL(const char))NN_OF_DIR(q) + ((size_t)batch * nq + qfirst) * sizeof(NNPoint);
    GENPC_TL(8);
#pragma unroll
    for (int r = 0; r < Q; r++) {
        int j = q0 + r * 32;
        if (j >= nq) j = nq - 1;
        const NNPoint p = nn_load_point(q_base, (unsigned)(j - qfirst) * (unsigned)sizeof(NNPoint));
        raw0[r] = half ? p.z : p.x;
        raw1[r] = p.y;
    }
    // (A per-launch pre-pass that hands every block its batch element's scale -- so that a slice longer than an LDS tile is
    // not read twice -- was measured: 13 x 16384^2 280.5 -> 278.9 us, 4 x 16384 x 8192 54.0 -> 58.2: the pre-scan of a
    // multi-round launch hides behind the other resident blocks, the extra launch does not.)
    // raw coordinates of an LDS tile, HT / kBlock targets per thread.  A slice that fits one LDS tile (HT = 2048 at
    // 1 x 16384^2) is read from memory ONCE: the registers that feed the scale's maximum also feed the staging,
    // and the whole slice is staged behind a single barrier pair (with 1024-target tiles a block spent 43 % of its
    // time outside the MFMA loop: 3 us on this pass, 2 us re-reading tile 0, 2 us staging tile 1 between the loops
    // with every wave waiting for the slowest -- tools/nn_timeline.py).
    constexpr int kPer = HT / kThreads;
    float pre[kPer][3];
    // later copies of a bit-identical target (nn_dedupe.hip; bit i: this thread's i-th target of the tile) are staged like
    // padding: the first copy answers for them, and three equal minima in one list would send the query to the exhaustive pass
    const unsigned *__restrict__ dupm = dup_dir ? dup_dir + (dup_shared ? (size_t)0 : (size_t)batch * ((nt + 31) >> 5)) : nullptr;
    unsigned predup = 0u;
    const auto t_base = (NN_GLOBAL(const char))NN_OF_DIR(t) + (size_t)batch * nt * sizeof(NNPoint);
    auto prefetch = [&](int t0) {
        predup = 0u;
        int tc[kPer];
#pragma unroll
        for (int i = 0; i < kPer; i++) {
            const int t = t0 + i * kThreads + threadIdx.x;
            tc[i] = t < nt ? t : nt - 1;
            // (12 tc below 2^32: the plan keeps clouds of 2^25 targets and more away from this kernel)
            const NNPoint p = nn_load_point(t_base, (unsigned)tc[i] * (unsigned)sizeof(NNPoint));
            pre[i][0] = p.x;
            pre[i][1] = p.y;
            pre[i][2] = p.z;
        }
        if (dupm) {
            // all mask words first, then their bits: no wait per target
            unsigned mw[kPer];
#pragma unroll
            for (int i = 0; i < kPer; i++) mw[i] = dupm[tc[i] >> 5];
#pragma unroll
            for (int i = 0; i < kPer; i++) predup |= ((mw[i] >> (tc[i] & 31)) & 1u) << i;
        }
    };
    const bool resident = k_end - k_begin <= HT;        // block-uniform
    // A resident slice that fills the LDS tile and has no duplicate mask -- every slice of a call whose clouds are multiples
    // of the slice length, 1 x 16384^2 among them -- is reduced and staged in a straight line: no padding rows, no mask
    // bits, no predicate per target (block-uniform, as are `resident` and `publishes`).
    // (The loads are the same on both paths, clamp included: a second set of loads behind a branch made the compiler wait for
    // the query loads at the point where the two met.)
    // (the three-wave form with two lists per lane is held to 168 VGPRs with 128 B of scratch; the second staging path cost
    // it 4 B more, so it keeps the general one)
    constexpr bool kStraight = !(W == 3 && NL == 2);
    const bool full = kStraight && k_end - k_begin == HT && !dupm;
    // every query block of a slice sees the same targets: the first one alone works out and publishes their max |t'|^2
    const bool publishes = qb == 0;
    if (resident && k_begin < k_end) prefetch(k_begin);
    // centred queries of this lane; the block's largest |coordinate| over queries and slice
    float qc0[Q], qc1[Q];
    float mx = 0.0f;
#pragma unroll
    for (int r = 0; r < Q; r++) {
        qc0[r] = raw0[r] - (half ? cz : cx);
        qc1[r] = half ? 0.0f : raw1[r] - cy;
        // a query at infinity is answered by the exhaustive pass; it must not set the block's scale
        const float m0 = fabsf(qc0[r]), m1 = fabsf(qc1[r]);
        mx = fmaxf(mx, fmaxf(m0 < __builtin_inff() ? m0 : 0.0f, m1 < __builtin_inff() ? m1 : 0.0f));
    }
    if (full) {
#pragma unroll
        for (int i = 0; i < kPer; i++)
            mx = fmaxf(mx, fmaxf(fmaxf(fabsf(pre[i][0] - cx), fabsf(pre[i][1] - cy)), fabsf(pre[i][2] - cz)));
    } else if (resident) {
#pragma unroll
        for (int i = 0; i < kPer; i++)
            if (k_begin + i * kThreads + (int)threadIdx.x < k_end)
                mx = fmaxf(mx, fmaxf(fmaxf(fabsf(pre[i][0] - cx), fabsf(pre[i][1] - cy)), fabsf(pre[i][2] - cz)));
    } else {
        for (int t = k_begin + threadIdx.x; t < k_end; t += kThreads) {
            const float *tp = T + (size_t)t * 3;
            mx = fmaxf(mx, fmaxf(fmaxf(fabsf(tp[0] - cx), fabsf(tp[1] - cy)), fabsf(tp[2] - cz)));
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (lane == 0) s_red[wave] = mx;
    __syncthreads();
    mx = s_red[0];
#pragma unroll
    for (int w2 = 1; w2 < WV; w2++) mx = fmaxf(mx, s_red[w2]);
    GENPC_TL(1);
    const float sc = scale_for(mx);             // NaN input: comparisons fail -> 1
    const float isc = 1.0f / sc;                 // exact (power of two)
    const float tsc = -2.0f * sc;

    h16x8 bq[Q];
    Top3 lst[Q][NL];
#pragma unroll
    for (int r = 0; r < Q; r++) {
        const unsigned p0 = split2(qc0[r] * sc), p1 = split2(qc1[r] * sc);
        // [h,l,h,l | h,l,h,l]; lanes >= 32: z pieces, then 2^8 twice (f16 0x5c00), zeros
        const uint4 v = half ? make_uint4(p0, p0, 0x5c005c00u, 0u) : make_uint4(p0, p0, p1, p1);
        bq[r] = __builtin_bit_cast(h16x8, v);
#pragma unroll
        for (int n = 0; n < NL; n++) top3_init(lst[r][n]);
    }

    // One accumulator per query tile, all on the same 32-target tile.  The rows of the next
    // two tiles are in registers (set p = tile parity) while the current tile's
    // accumulators are reduced.
    f32x16 acc[Q];
    uint4 A[2];
    auto fetch = [&](int p, int row) { A[p] = plane[half][row + col]; };
    auto mm = [&](int p, int r) {
        const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        acc[r] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, A[p]), bq[r], z, 0, 0, 0);
    };
    // One target tile (index parity p): fold the accumulators of tile `row` into the running
    // unit minima (four independent chains per query tile) and start tile row + 32 (set
    // p^1): slot r = 8 v_min3(acc[r]) | MFMA(r).  No branches: the last tile of an LDS tile
    // uses `last` (reduce only); fetches past the end read the spare rows.
    auto step = [&](auto p_tag, auto last_tag, int row, float (&m)[Q][4]) {
        constexpr int p = decltype(p_tag)::value;
        constexpr bool last = decltype(last_tag)::value;
        if (!last) fetch(p, row + 64);
        if (Q == 2) asm volatile("s_nop 3");      // 8 v_min3 + MFMA + ds_read = 10 wait states, 11 needed
#pragma unroll
        for (int r = 0; r < Q; r++) {
            const f32x16 &c = acc[r];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < 16; e += 2)
                asm("v_min3_f32 %0, %1, %2, %3" : "=v"(m[r][(e >> 1) & 3]) : "v"(m[r][(e >> 1) & 3]), "v"(c[e]), "v"(c[e + 1]));
            __builtin_amdgcn_sched_barrier(0);
            if (!last) mm(p ^ 1, r);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    float tmax2 = 0.0f;
    float nf = 0.0f;      // NaN once a target of the slice had a non-finite coordinate
    if (!resident && k_begin < k_end) prefetch(k_begin);
    for (int t0 = k_begin; t0 < k_end && !(debug & 4); t0 += HT) {
        const int tn = min(HT, k_end - t0);
        const int tn_pad = (tn + kC - 1) / kC * kC;
        __syncthreads();                 // every wave is done reading the previous tile
        // the two rows of target i of this thread: centre, scale, two f16 pieces of -2s x', -2s y', -2s z', s^2 |t'|^2 2^-8
        auto rows_of = [&](int i, uint4 &V0, uint4 &V1) {
            const float x = pre[i][0] - cx, y = pre[i][1] - cy, z = pre[i][2] - cz;
            const float xs = x * sc, ys = y * sc, zs = z * sc;
            const float tts = __fmaf_rn(zs, zs, __fmaf_rn(ys, ys, __fmul_rn(xs, xs)));
            const unsigned px = split2(x * tsc), py = split2(y * tsc), pz = split2(z * tsc);
            const unsigned pt = split2(tts * 0.00390625f);
            V0 = make_uint4(dup_lo(px), dup_hi(px), dup_lo(py), dup_hi(py));
            V1 = make_uint4(dup_lo(pz), dup_hi(pz), pt, 0u);
        };
        // ... and what it adds to max |t'|^2 and the non-finite flag (unscaled, centred: the finish step's threshold is made of it)
        auto measure = [&](int i) {
            const float x = pre[i][0] - cx, y = pre[i][1] - cy, z = pre[i][2] - cz;
            const float tt = __fmaf_rn(z, z, __fmaf_rn(y, y, __fmul_rn(x, x)));
            tmax2 = fmaxf(tmax2, tt);
            nf = __fmaf_rn(tt, 0.0f, nf);        // inf x 0 = NaN, NaN sticks (v_max drops NaNs)
        };
        if (full) {
#pragma unroll
            for (int i = 0; i < kPer; i++) {
                const int t = i * kThreads + threadIdx.x;
                uint4 V0, V1;
                rows_of(i, V0, V1);
                const int row = (t & ~31) | tile_row(t & 31);
                plane[0][row] = V0;
                plane[1][row] = V1;
            }
            if (publishes) {
#pragma unroll
                for (int i = 0; i < kPer; i++) measure(i);
            }
        } else {
#pragma unroll
            for (int i = 0; i < kPer; i++) {
                const int t = i * kThreads + threadIdx.x;
                if (t < tn_pad) {
                    uint4 V0, V1;
                    rows_of(i, V0, V1);
                    if (t >= tn || ((predup >> i) & 1u)) {
                        // padding: |t'|^2 = +inf (f16 0x7c00) x 2^8 never wins, the other terms are 0
                        V0 = make_uint4(0u, 0u, 0u, 0u);
                        V1 = make_uint4(0u, 0u, 0x7c00u, 0u);
                    } else if (publishes) {
                        measure(i);
                    }
                    const int row = (t & ~31) | tile_row(t & 31);
                    plane[0][row] = V0;
                    plane[1][row] = V1;
                }
            }
            if (t0 + HT < k_end) prefetch(t0 + HT);
        }
        __syncthreads();
        if (t0 == k_begin) { GENPC_TL(2); GENPC_TL_PARTNER(9); } else GENPC_TL(3);
        // prologue of the LDS tile: target tile 0, rows of tiles 0 and 1
        fetch(0, 0);
        fetch(1, 32);
#pragma unroll
        for (int r = 0; r < Q; r++) mm(0, r);
        asm volatile("s_nop 15");           // wait states before the first inline-asm read of acc[0]
        for (int rb0 = 0; rb0 < tn_pad; rb0 += NL * kC) {
#pragma unroll
            for (int n = 0; n < NL; n++) {
                const int rb = rb0 + n * kC;
                if (rb < tn_pad) {
                    float m[Q][4];
#pragma unroll
                    for (int r = 0; r < Q; r++) m[r][0] = m[r][1] = m[r][2] = m[r][3] = __builtin_inff();
#pragma unroll
                    for (int g = 0; g < U - 1; g++) {
                        if (g & 1) step(std::integral_constant<int, 1>{}, std::false_type{}, rb + 32 * g, m);
                        else step(std::integral_constant<int, 0>{}, std::false_type{}, rb + 32 * g, m);
                    }
                    // U is even: the last tile of a unit has parity 1
                    if (rb + kC < tn_pad) step(std::integral_constant<int, 1>{}, std::false_type{}, rb + kC - 32, m);
                    else step(std::integral_constant<int, 1>{}, std::true_type{}, rb + kC - 32, m);
#pragma unroll
                    for (int r = 0; r < Q; r++) {
                        float v;
                        asm("v_min3_f32 %0, %1, %2, %3" : "=v"(v) : "v"(m[r][0]), "v"(m[r][1]), "v"(m[r][2]));
                        asm("v_min_f32 %0, %1, %2" : "=v"(v) : "v"(v), "v"(m[r][3]));
                        top3_insert(lst[r][n], v, t0 + rb + half);      // scaled value; bit 0: which 16 rows of each tile
                    }
                }
            }
        }
    }

    GENPC_TL(4);
    GENPC_TL_PARTNER(10);
    // max |t'|^2 of the slice, for the bound of the finish step: every query block sees the same targets, the
    // first one publishes
    if (publishes) {
        // non-finite targets: +inf tells the finish step to answer every query of this cloud
        // exhaustively (the reference's tile semantics for NaNs, nn_exhaustive in nn.h)
        if (nf != nf) tmax2 = __builtin_inff();
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) tmax2 = fmaxf(tmax2, __shfl_xor(tmax2, o));
        __syncthreads();
        if (lane == 0) s_red[wave] = tmax2;
        __syncthreads();
        float tm = s_red[0];
#pragma unroll
        for (int w2 = 1; w2 < WV; w2++) tm = fmaxf(tm, s_red[w2]);
        if (threadIdx.x == 0) tmaxp_dir[(size_t)batch * slices + slice] = tm;
    }

    // Publish the lists: the two lane halves folded, NL lists of one 16-byte record per query and slice
    // (a1, c1) (codes of a2 and a3, c2): list_enc and ListRec in nn.h.  One 16-byte store per list: the 32 lanes that store
    // write 512 contiguous bytes.
    // The halves share the work: of the wave's Q query tiles, lanes 0-31 merge, encode and store the first Q / 2, lanes 32-63 the
    // others, tile r beside tile r + Q / 2 in one pass -- all 64 lanes store, and each tile's instructions run once per pair.
    const size_t bnq = (size_t)nbatch * nq;
    constexpr int QH = Q / 2;
    static_assert(Q % 2 == 0, "the lane halves take half of the query tiles each");
    // v_permlane32_swap: lanes 32-63 of a <-> lanes 0-31 of b (the compiler supplies the instruction's wait states).
    // The two results go into scalars before they are cast: __builtin_bit_cast applied to an ELEMENT of the result vector,
    // __builtin_bit_cast(float, v[1]), reads element 0 whichever is named -- half of all nearest neighbours were wrong that way.
    auto swap_word = [](auto &a, auto &b) {
        const auto v = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b), false, false);
        const unsigned va = v[0], vb = v[1];
        a = __builtin_bit_cast(std::remove_reference_t<decltype(a)>, va);
        b = __builtin_bit_cast(std::remove_reference_t<decltype(b)>, vb);
    };
    auto swap_halves = [&](Top3 &a, Top3 &b) {
        swap_word(a.a1, b.a1);
        swap_word(a.a2, b.a2);
        swap_word(a.a3, b.a3);
        swap_word(a.c1, b.c1);
        swap_word(a.c2, b.c2);
    };
#pragma unroll
    for (int r = 0; r < QH; r++) {
#pragma unroll
        for (int n = 0; n < NL; n++) {
            Top3 &f = lst[r][n], &o = lst[r + QH][n];
            // unscale (the block's scale is one power of two, so the order was not affected):
            // s^2 (|t'|^2 - 2 q'.t') -> |t'|^2 - 2 q'.t', two exact multiplications
            f.a1 = (f.a1 * isc) * isc;
            f.a2 = (f.a2 * isc) * isc;
            f.a3 = (f.a3 * isc) * isc;
            o.a1 = (o.a1 * isc) * isc;
            o.a2 = (o.a2 * isc) * isc;
            o.a3 = (o.a3 * isc) * isc;
            // f held tile r and o tile r + QH, each lane its own half's rows.  Swapped, f is in every lane what lanes 0-31
            // found for the lane's tile of the pair and o what lanes 32-63 found for it: the merge below is, in both halves,
            // the one lanes 0-31 alone used to run for each tile -- their list first, the other half's entries inserted in order.
            swap_halves(f, o);
            top3_insert(f, o.a1, o.c1);
            top3_insert(f, o.a2, o.c2);
            top3_insert(f, o.a3, -1);
            const int j = q0 + (r + QH * half) * 32;
            if (j < nq) {
                const unsigned code2 = list_enc(f.a1, f.a2);
                const unsigned code3 = list_enc(list_dec(f.a1, code2), f.a3);
                ListRec rec;
                rec.x = ((unsigned long long)__float_as_uint(f.a1) << 32) | (unsigned)f.c1;
                rec.y = ((unsigned long long)((code2 << 16) | code3) << 32) | (unsigned)f.c2;
                // the block's first record of this list: a scalar base, the lane adds 16 (j - qfirst) to it
                ListRec *p = list_rec(part_dir, slice * NL + n, bnq, batch, nq, qfirst);
                // written through (sc1): a block's 16 KB of lists are on their way to memory when they are stored, not when the
                // kernel's end finds them dirty in the L2 -- and the finish blocks read them from other XCDs in any case.
                // (The filter's trace duration minus its last block's end, 1 x 16384^2: plain 3.0 us, non-temporal 2.8,
                // written through 2.2, the finish kernel unchanged; DESIGN_NOTEBOOK.md, "list records".)  Written as the
                // instruction: a plain 16-byte store cannot carry the bit; the s_nop keeps the next instruction off the data registers.
                asm volatile("global_store_dwordx4 %0, %1, %2 sc1\n\ts_nop 1"
                             : : "v"((unsigned)(j - qfirst) * (unsigned)sizeof(ListRec)), "v"(rec), "s"((NN_GLOBAL(ListRec))p) : "memory");
            }
        }
    }
    GENPC_TL(5);
    GENPC_TL_PARTNER(11);
}

template <int Q, int NL>
static void launch_main(const NNArgs &a, const NNPlan &plan, hipStream_t st, hipEvent_t e0, hipEvent_t e1)
{
    // (e0 / e1: genpc_nn_profile -- the events ride on the kernel's own dispatch, hipExtLaunchKernelGGL: they take the dispatch's
    //  start and end timestamps, what a rocprofv3 kernel trace reports, not the interval between two marker packets around it)
#define NN_F16_LAUNCH(KERNEL, GRID, BLOCK)                                                                              \
    do {                                                                                                                \
        if (e0) hipExtLaunchKernelGGL(KERNEL, GRID, BLOCK, 0, st, e0, e1, 0, a);                                        \
        else hipLaunchKernelGGL(KERNEL, GRID, BLOCK, 0, st, a);                                                         \
    } while (0)
    // the forms of the 512-query blocks (nn_plan.h NNForm: waves per block, resident blocks per CU, LDS tile); 256-query
    // blocks have the four-wave form alone.  plan.unit is 2 or 4.
    const int blocks = (int)plan.blocks;
    if (Q == 4 && plan.form == kNNWide) {
        if (plan.unit == 2) NN_F16_LAUNCH((nn_f16_kernel<4, 2, NL, 1, 2 * kHTile, 8>), dim3(blocks), dim3(8 * kWave));
        else NN_F16_LAUNCH((nn_f16_kernel<4, 4, NL, 1, 2 * kHTile, 8>), dim3(blocks), dim3(8 * kWave));
    } else if (Q == 4 && plan.form == kNNTile2048) {
        if (plan.unit == 2) NN_F16_LAUNCH((nn_f16_kernel<4, 2, NL, 2, 2 * kHTile, 4>), dim3(blocks), dim3(kBlock));
        else NN_F16_LAUNCH((nn_f16_kernel<4, 4, NL, 2, 2 * kHTile, 4>), dim3(blocks), dim3(kBlock));
    } else if (Q == 4 && plan.form == kNNThreeWave) {
        if (plan.unit == 2) NN_F16_LAUNCH((nn_f16_kernel<Q, 2, NL, (Q == 4 ? 3 : 4), kHTile, 4>), dim3(blocks), dim3(kBlock));
        else NN_F16_LAUNCH((nn_f16_kernel<Q, 4, NL, (Q == 4 ? 3 : 4), kHTile, 4>), dim3(blocks), dim3(kBlock));
    } else {
        if (plan.unit == 2) NN_F16_LAUNCH((nn_f16_kernel<Q, 2, NL, (Q == 4 ? 2 : 4), kHTile, 4>), dim3(blocks), dim3(kBlock));
        else NN_F16_LAUNCH((nn_f16_kernel<Q, 4, NL, (Q == 4 ? 2 : 4), kHTile, 4>), dim3(blocks), dim3(kBlock));
    }
#undef NN_F16_LAUNCH
}

// genpc_nn_profile(): HIP events ON the filter kernel's dispatch (bench.py's roofline line).  Per calling host thread (round 4
// kept this state process-wide: a lane that profiled raced every other lane's launches -- VERDICT r4 weak #13): only the
// launches of the thread that asked are bracketed, with that thread's own pair of events.
static thread_local bool g_prof_on = false;
static thread_local hipEvent_t g_prof_e0 = nullptr, g_prof_e1 = nullptr;

// Launches the filter and the finish kernel: maps the plan to a template instance, decides nothing.
int launch_nn_f16(NNArgs &a, const NNPlan &plan, hipStream_t st)
{
    WsLayout L;
    for (int d = 0; d < a.ndir; d++) L.add(a.dir[d].tmaxp, (size_t)a.b * a.dir[d].ntmax);
    if (!ws_alloc(L, kWsNnTmax, st)) return 0;
    hipEvent_t pe0 = nullptr, pe1 = nullptr;
    if (g_prof_on) {
        if (!g_prof_e0) { (void)hipEventCreate(&g_prof_e0); (void)hipEventCreate(&g_prof_e1); }
        pe0 = g_prof_e0;
        pe1 = g_prof_e1;
    }
    // (256-target bookkeeping units, U = 8, in the wide form: filter -0.4 us, finish +1.7 us at 1 x 16384^2 -- not kept)
    if (plan.q == 4) {
        if (plan.nl == 2) launch_main<4, 2>(a, plan, st, pe0, pe1);
        else launch_main<4, 1>(a, plan, st, pe0, pe1);
    } else {
        if (plan.nl == 2) launch_main<2, 2>(a, plan, st, pe0, pe1);
        else launch_main<2, 1>(a, plan, st, pe0, pe1);
    }
    if (!check(hipGetLastError(), "nn_f16_kernel launch")) return 0;
    return launch_nn_finish(a, plan, (float)kQTh, (float)kTTh, 0.0f, st);
}

}  // namespace genpc

#ifdef GENPC_NN_TIMELINE
extern "C" __attribute__((visibility("default"))) int genpc_nn_timeline_read(unsigned long long *out)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(genpc::g_timeline), sizeof(unsigned long long) * 4096 * genpc::kTimelineRow) == hipSuccess;
}
#endif

GENPC_API float genpc_nn_profile(int enable)
{
    using namespace genpc;
    float ms = -1.0f;
    if (g_prof_on && g_prof_e1 && hipEventSynchronize(g_prof_e1) == hipSuccess) (void)hipEventElapsedTime(&ms, g_prof_e0, g_prof_e1);
    g_prof_on = enable != 0;
    return ms;
}
