// chamfer.hip -- brute-force nearest neighbour (Chamfer3D forward/backward) for
// gfx950.  Replaces loss_functions/Chamfer3D/chamfer3D.cu of the reference.
//
// Forward design.  The kernel is VALU-bound (6.5 kflop per HBM byte).
// Measured issue model on MI355X (tools/ubench_valu.hip): v_fma/v_mul/v_add/v_sub
// f32 with VGPR operands issue at ~105 lane-ops/clk/CU; every instruction with an
// SGPR operand, v_min/v_min3/v_cmp/v_cndmask, packed-f32 and f64 ops issue at half
// of that.  Hence:
//   * a lane owns R queries in VGPRs; targets are staged per block in LDS (groups
//     of four as x0..x3|y0..y3|z0..z3) and read with uniform-address (broadcast)
//     ds_read_b128 -- three reads deliver four targets -- so that the
//     three subtractions per pair keep VGPR operands and stay full rate (fetching
//     the wave-uniform targets through the scalar cache as SGPR operands costs 10
//     issue units per pair instead of 7 -- measured 1.4x slower at large batch);
//   * the inner loop tracks only the minimum VALUE of a chunk of kChunk targets
//     (one v_min3 per two pairs); per tile the chunk that produced a new minimum
//     is re-scanned in LDS to recover the FIRST index attaining it, which is the
//     reference's strict-'<' tie-break (chamfer3D.cu:36,46,56,66,119,126);
//     per pair: 3 sub + mul + 2 fma (full rate) + 1/2 min3 (half rate) = 7 units;
//   * both directions (A->B, B->A), all batch elements, all query blocks and all
//     target slices are ONE launch sized from the problem (the reference's fixed
//     32x16 grid leaves 94 % of an MI355X idle at B=1); the running minimum never
//     leaves registers (the reference read-modify-writes result[] in global
//     memory every 512 targets);
//   * when targets are split into S>1 slices for occupancy, per-slice
//     (min,argmin) go to scratch and the LAST block to finish a query block folds
//     them in slice order with strict '<' (earlier slice == lower index wins), so
//     results do not depend on S and no second launch is needed.  The hand-off is
//     the agent-scope release -> ticket -> acquire recipe (per-XCD L2s are not
//     coherent with each other).
// Arithmetic is written with explicit __fmaf_rn/__fmul_rn/__fadd_rn and the file
// is compiled with -ffp-contract=off, so the compiler cannot re-associate or
// contract differently from oracle/genpc_oracle.c.
#include "nn.h"
#include "../../include/genpc_hip.h"

#include <stdlib.h>
#include <algorithm>
#include <atomic>
#include <mutex>

namespace genpc {

constexpr int kTile = 2048;      // targets per LDS tile (24 KiB: 12 B per target)




// One block = one (direction, target slice, batch, 256*R-query block) unit; wave w
// of the block owns queries [w*64*R, (w+1)*64*R) of that block.
template <int R, int FMA>
__global__ __launch_bounds__(kBlock) void nn_forward_kernel(NNArgs a)
{
    __shared__ float4 tile[kTile / 4 * 3 + 3];      // + one spare group for the pipeline's last prefetch
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    // every kernel argument the block uses, in one round (nn.h, above NN_ARG); the decode divides by multiplying (nn_decode.h)
    int ndir = a.ndir, nbatch = a.b, slice_len = a.slice_len, debug = a.debug;
    NNDiv by_b = a.by_b;
    NN_GLOBAL(int) arrive_g = (NN_GLOBAL(int))a.arrive;
    NN_ARG(int, begin, block_begin); NN_ARG(int, qblocks, qblocks); NN_ARG(NNDiv, by_q, by_qblocks);
    NN_ARG(int, nq, nq); NN_ARG(int, nt, nt); NN_ARG(int, slices, slices); NN_ARG(int, ubegin, unit_begin);
    NN_ARG_PTR(const float, q, q); NN_ARG_PTR(const float, t, t);
    NN_ARG_PTR(float, out_d, out_d); NN_ARG_PTR(int, out_i, out_i); NN_ARG_PTR(unsigned long long, part, part);
    asm volatile("" : "+s"(ndir), "+s"(nbatch), "+s"(slice_len), "+s"(debug), "+s"(by_b.mul), "+s"(by_b.shift), "+s"(arrive_g),
                 NN_HELD(begin), NN_HELD(qblocks), "+s"(by_q_0.mul), "+s"(by_q_0.shift), "+s"(by_q_1.mul), "+s"(by_q_1.shift), NN_HELD(nq), NN_HELD(nt),
                 NN_HELD(slices), NN_HELD(ubegin), NN_HELD(q), NN_HELD(t), NN_HELD(out_d), NN_HELD(out_i), NN_HELD(part));
    int *const arrive = (int *)arrive_g;
    const int d = (ndir > 1 && (int)blockIdx.x >= begin_1) ? 1 : 0;
    const int qblocks = NN_OF_DIR(qblocks), nq = NN_OF_DIR(nq), nt = NN_OF_DIR(nt), slices = NN_OF_DIR(slices), unit_begin = NN_OF_DIR(ubegin);
    const float *const q_dir = (const float *)NN_OF_DIR(q), *const t_dir = (const float *)NN_OF_DIR(t);
    float *const out_d_dir = (float *)NN_OF_DIR(out_d);
    int *const out_i_dir = (int *)NN_OF_DIR(out_i);
    unsigned long long *const part_dir = (unsigned long long *)NN_OF_DIR(part);
    // block id within the direction = (slice * b + batch) * qblocks + qblock
    const NNBlockId id = nn_decode_block((int)blockIdx.x - NN_OF_DIR(begin), qblocks, NNDiv{NN_OF_DIR(by_q).mul, NN_OF_DIR(by_q).shift}, nbatch, by_b);
    const int qb = id.qb, batch = id.batch, slice = id.slice;

    const float *__restrict__ Q = q_dir + (size_t)batch * nq * 3;
    const float *__restrict__ T = t_dir + (size_t)batch * nt * 3;

    const int k_begin = slice * slice_len;
    int k_end = k_begin + slice_len;
    if (k_end > nt) k_end = nt;

    float qx[R], qy[R], qz[R], best[R];
    int bchunk[R];
    const int q0 = (qb * kWavesPerBlock + wave) * (kWave * R) + lane;
#pragma unroll
    for (int r = 0; r < R; r++) {
        int j = q0 + r * kWave;
        if (j >= nq) j = nq - 1;
        qx[r] = Q[(size_t)j * 3 + 0];
        qy[r] = Q[(size_t)j * 3 + 1];
        qz[r] = Q[(size_t)j * 3 + 2];
        best[r] = __builtin_inff();
        bchunk[r] = k_begin;
    }

    // LDS tile layout: groups of 4 targets as three float4s (x0..x3 | y0..y3 | z0..z3),
    // so that every byte a ds_read_b128 fetches is used (12 B per target).
    float *tile_f = (float *)tile;
    float nf = 0.0f;      // NaN once a target of the slice had a non-finite coordinate
    for (int t0 = k_begin; t0 < k_end && !(debug & 4); t0 += kTile) {
        const int tn = min(kTile, k_end - t0);
        const int tn_pad = (tn + kChunk - 1) / kChunk * kChunk;
        __syncthreads();                       // readers of the previous tile are done
        for (int t = threadIdx.x; t < tn_pad; t += kBlock) {
            float x, y, z;
            if (t < tn) {
                const float *tp = T + (size_t)(t0 + t) * 3;
                x = tp[0]; y = tp[1]; z = tp[2];
                nf = __fmaf_rn((fabsf(x) + fabsf(y)) + fabsf(z), 0.0f, nf);      // inf x 0 = NaN, NaN sticks
            } else {
                // pad the ragged tail of the last chunk: a +inf distance never wins a strict '<'
                x = y = z = __builtin_inff();
            }
            float *g = tile_f + (t >> 2) * 12 + (t & 3);
            g[0] = x; g[4] = y; g[8] = z;
        }
        __syncthreads();

        // Software pipeline: the three reads of group g+1 are issued before the
        // VALU work of group g (the scheduler otherwise sinks each read next to its
        // first use and every group eats a full LDS round trip).
        float4 X = tile[0], Y = tile[1], Z = tile[2];
        for (int c0 = 0; c0 < tn_pad; c0 += kChunk) {
            const float4 *tl = tile + (c0 >> 2) * 3;
            float m[R];
#pragma unroll
            for (int r = 0; r < R; r++) m[r] = __builtin_inff();
#pragma unroll
            for (int g = 0; g < kChunk / 4; g++) {
                // one group past the end of the last chunk is read and dropped (the
                // array has a spare group)
                const float4 Xn = tl[g * 3 + 3], Yn = tl[g * 3 + 4], Zn = tl[g * 3 + 5];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const float d0 = sqdist<FMA>(X.x - qx[r], Y.x - qy[r], Z.x - qz[r]);
                    const float d1 = sqdist<FMA>(X.y - qx[r], Y.y - qy[r], Z.y - qz[r]);
                    const float d2 = sqdist<FMA>(X.z - qx[r], Y.z - qy[r], Z.z - qz[r]);
                    const float d3 = sqdist<FMA>(X.w - qx[r], Y.w - qy[r], Z.w - qz[r]);
                    m[r] = fminf(fminf(m[r], d0), d1);
                    m[r] = fminf(fminf(m[r], d2), d3);
                }
                __builtin_amdgcn_sched_barrier(0);
                X = Xn; Y = Yn; Z = Zn;
            }
#pragma unroll
            for (int r = 0; r < R; r++) {
                const bool lt = m[r] < best[r];
                best[r] = lt ? m[r] : best[r];
                bchunk[r] = lt ? t0 + c0 : bchunk[r];
            }
        }
    }

    // Non-finite input: the minimum-of-chunks scan silently skips NaN distances, the reference's
    // tiled scan does not always (nn_exhaustive, nn.h).  A slice that saw a non-finite target marks
    // its partials; queries of such a cloud, and non-finite queries, are answered exhaustively.
    int *s_or = (int *)tile + 12;              // block_or's four words: beside the exhaustive pass's, which use the tile below
    int bad = block_or(nf != nf, s_or);
    if (slices > 1) {
        // Publish this slice's (minimum, chunk) per query; the last block to arrive for
        // this (direction, batch, query block) folds all S slices in slice order with
        // strict '<' (earlier slice == lower index wins) and carries on alone.
        // The partial (minimum, chunk) of a query is ONE 8-byte word, stored and loaded
        // with agent-scope atomics (write-through `sc1` stores, L1-bypassing loads): with
        // 8-byte agent atomics on both sides no release / acquire fence is needed -- a
        // release would write back the whole XCD's dirty L2 lines.
        const size_t bnq = (size_t)nbatch * nq;
        unsigned long long *P = part_dir + (size_t)batch * nq;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int j = q0 + r * kWave;
            if (j < nq) {
                const unsigned long long v = bad ? ~0ull : ((unsigned long long)__float_as_uint(best[r]) << 32) | (unsigned)bchunk[r];
                __hip_atomic_store(P + (size_t)slice * bnq + j, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (debug & 2) return;
        int *cnt = arrive + unit_begin + batch * qblocks + qb;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int *s_ticket = (int *)tile;      // the tile is dead after the barrier above (one LDS object)
        if (threadIdx.x == 0)
            *s_ticket = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (*s_ticket != slices - 1) return;
        if (threadIdx.x == 0) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
#pragma unroll
        for (int r = 0; r < R; r++) {
            int j = q0 + r * kWave;
            j = j < nq ? j : nq - 1;
            unsigned long long v = __hip_atomic_load(P + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            bad |= v == ~0ull;
            float bv = __uint_as_float((unsigned)(v >> 32));
            int bc = (int)(unsigned)v;
            if (v == ~0ull) { bv = __builtin_inff(); bc = 0; }      // marked slice: no chunk to recover (the query goes exhaustive)
            for (int s2 = 1; s2 < slices; s2++) {
                v = __hip_atomic_load(P + (size_t)s2 * bnq + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                bad |= v == ~0ull;
                const float vv = __uint_as_float((unsigned)(v >> 32));
                const bool lt = vv < bv;
                bv = lt ? vv : bv;
                bc = lt ? (int)(unsigned)v : bc;
            }
            best[r] = bv;
            bchunk[r] = bc;
        }
    }

    // Recover the FIRST index attaining best[r] inside the remembered chunk: same
    // operands, same operations => bitwise-equal distance.  Done once per query (by
    // the merging block when the targets were sliced), from global memory, as 24
    // 16-byte loads per query.  Positions past the end of the cloud are clamped to
    // its last target; positions past the end of the chunk's slice belong to the
    // next slice.  Either can only match at a HIGHER position than the true first
    // index, which lies inside the slice, and the lowest match wins.
    typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
    float *__restrict__ od = out_d_dir + (size_t)batch * nq;
    int *__restrict__ oi = out_i_dir + (size_t)batch * nq;
    // the target tile is dead: its LDS holds the list of queries for the exhaustive pass
    __syncthreads();
    int *s_nflag = (int *)tile;
    int *s_xfi = s_nflag + 4;
    float *s_xred = (float *)(s_nflag + 8);
    int *s_flag = s_nflag + 16;                  // up to kBlock * R entries
    if (threadIdx.x == 0) *s_nflag = 0;
    bad = block_or(bad, s_or);                   // merged partials: every lane read the same marks
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int base = bchunk[r];
        int first = 0;
        if (!(debug & 1)) {
            if (base + kChunk <= nt) {
                const f4u *tp = (const f4u *)(T + (size_t)base * 3);
#pragma unroll
                for (int c8 = kChunk - 8; c8 >= 0; c8 -= 8) {
                    f4u v[6];
#pragma unroll
                    for (int i = 0; i < 6; i++) v[i] = tp[(c8 >> 2) * 3 + i];
                    const float f[24] = {v[0].x, v[0].y, v[0].z, v[0].w, v[1].x, v[1].y, v[1].z, v[1].w,
                                         v[2].x, v[2].y, v[2].z, v[2].w, v[3].x, v[3].y, v[3].z, v[3].w,
                                         v[4].x, v[4].y, v[4].z, v[4].w, v[5].x, v[5].y, v[5].z, v[5].w};
#pragma unroll
                    for (int c = 7; c >= 0; c--) {
                        const float dd = sqdist<FMA>(f[c * 3 + 0] - qx[r], f[c * 3 + 1] - qy[r], f[c * 3 + 2] - qz[r]);
                        first = (dd == best[r]) ? c8 + c : first;
                    }
                }
            } else {
                for (int c = kChunk - 1; c >= 0; c--) {
                    int kk = base + c;
                    kk = kk < nt ? kk : nt - 1;
                    const float *tp = T + (size_t)kk * 3;
                    const float dd = sqdist<FMA>(tp[0] - qx[r], tp[1] - qy[r], tp[2] - qz[r]);
                    first = (dd == best[r]) ? c : first;
                }
            }
        }
        const int j = q0 + r * kWave;
        const bool qbad = !((fabsf(qx[r]) + fabsf(qy[r])) + fabsf(qz[r]) < __builtin_inff());
        if (j < nq) {
            if (bad || qbad) {
                s_flag[atomicAdd(s_nflag, 1)] = j;
            } else {
                od[j] = best[r];
                oi[j] = base + first;
            }
        }
    }
    __syncthreads();
    const int nflag = *s_nflag;
    for (int fidx = 0; fidx < nflag; fidx++) nn_exhaustive<FMA>(Q, T, nt, s_flag[fidx], od, oi, s_xred, s_xfi);
}

// ---------------------------------------------------------------------------
// MFMA path.  |q - t|^2 = |q|^2 + (|t|^2 - 2 q.t): the bracket is a K = 4 product of
// (qx, qy, qz, 1) with (-2tx, -2ty, -2tz, |t|^2), which v_mfma_f32_32x32x2_f32
// evaluates for 32 targets x 32 queries in two instructions (bitwise a k-ordered
// fmaf chain, MI355X guide) at the fp32 matrix rate -- 1024 pairs per 128 SIMD
// cycles, against ~7 issue units per pair on the VALU path.  The value is only an
// APPROXIMATION of the reference's fl((x2-x1)^2 + ...) (different roundings), so it
// is used as a filter with a rigorous error bound, never as the result:
//   * coordinates are centred on the target cloud's first point c (q' = fl(q - c),
//     t' = fl(t - c)), so magnitudes -- and the bound -- scale with the cloud's
//     extent, not with its offset from the origin;
//   * lane l of a wave holds, per MFMA pair, 16 approximate values of query l&31
//     against rows {8i + 4(l>>5) + 0..3} of a 32-target tile; it keeps the three
//     smallest minima over its (tile, half) units, with the tile index for two of them
//     (Top3); lanes l and l^32, then the target slices, fold their lists;
//   * with a1 <= a2 <= a3 the folded minima: every unit outside the first (first
//     two) listed tile(s) has approximate value >= a2 (a3).  nn_safe() proves from
//     the bound that the reference's minimum lies inside the listed tile(s); those
//     32 (64) targets are then evaluated with the reference's exact arithmetic, in
//     index order -> bitwise the reference's (distance, first index).  Queries for
//     which the proof fails (three tiles within the bound: exact ties on gridded
//     data, non-finite input) are re-done exhaustively by the merging block.
// Error bound, u = 2^-24, T = max |t'|, per target: the chain rounds four times on
// partial sums <= 2|q'||t'| + |t'|^2 and |t'|^2 itself carries 3 roundings, |q'|^2
// three: |a + |q'|^2 - |q' - t'|^2| <= E1 = u (8|q'|T + 7T^2 + 3|q'|^2); centring
// moves each point by <= u|p'|: |sqrt(D') - sqrt(D)| <= eta = u (|q'| + T); the
// reference's value is D (1 + theta), |theta| <= 6u (three subtractions, squared,
// three to five roundings of non-negative terms).  All evaluated in fp64 with u
// inflated by 1 %.
constexpr int kMTile = 2048;     // targets per LDS tile on the MFMA path (2 planes x 8 B)


// True when every target whose approximate value is >= a_rest provably has a
// reference distance above that of the target that produced a_best.
__device__ __forceinline__ bool nn_safe(float a_best, float a_rest, float qq, float tmax2)
{
    const double u = 1.01 * 5.9604644775390625e-8;
    const double T = sqrt((double)tmax2), qn = sqrt((double)qq);
    const double kSub = 64.0 * 1.401298464324817e-45;      // subnormal results round absolutely (see nn_tau)
    const double E1 = u * (8.0 * qn * T + 7.0 * T * T + 3.0 * (double)qq) + kSub;
    const double eta = u * (qn + T);
    double up = (double)a_best + (double)qq + E1;
    up = sqrt(up > 0.0 ? up : 0.0) + eta;
    up = up * up * (1.0 + 6.0 * u) + kSub;
    double lo = (double)a_rest + (double)qq - E1;
    lo = sqrt(lo > 0.0 ? lo : 0.0) - eta;
    lo = lo > 0.0 ? lo : 0.0;
    lo = lo * lo * (1.0 - 6.0 * u);
    return lo > up;      // false for NaN
}

// Exact (reference arithmetic) minimum and FIRST index over targets [base, base+len)
// of a cloud of nt targets, positions past the end clamped to the last target.

// One block = one (direction, target slice, batch, 128*Q-query block) unit; wave w
// owns Q tiles of 32 queries.  U = MFMA tiles per bookkeeping unit (re-scan
// granularity 32*U targets).
template <int Q, int U, int FMA>
__global__ __launch_bounds__(kBlock) void nn_mfma_kernel(NNArgs a)
{
    constexpr int kC = 32 * U;
    __shared__ float2 plane[2][kMTile + 2 * kC];  // + two spare units for the pipeline's last fetches
    __shared__ float s_red[kWavesPerBlock];
    __shared__ int s_fi[kWavesPerBlock];
    __shared__ int s_misc[2];                 // [0] arrival ticket, [1] number of flagged queries
    __shared__ int s_flag[kWavesPerBlock * Q * 32];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int half = lane >> 5, col = lane & 31;
    // every kernel argument the block uses, in one round (nn.h, above NN_ARG); the decode divides by multiplying (nn_decode.h)
    int ndir = a.ndir, nbatch = a.b, slice_len = a.slice_len, debug = a.debug;
    NNDiv by_b = a.by_b;
    NN_GLOBAL(int) arrive_g = (NN_GLOBAL(int))a.arrive;
    NN_GLOBAL(unsigned long long) stats_g = (NN_GLOBAL(unsigned long long))a.stats;
    NN_ARG(int, begin, block_begin); NN_ARG(int, qblocks, qblocks); NN_ARG(NNDiv, by_q, by_qblocks);
    NN_ARG(int, nq, nq); NN_ARG(int, nt, nt); NN_ARG(int, slices, slices); NN_ARG(int, ubegin, unit_begin);
    NN_ARG_PTR(const float, q, q); NN_ARG_PTR(const float, t, t);
    NN_ARG_PTR(float, out_d, out_d); NN_ARG_PTR(int, out_i, out_i); NN_ARG_PTR(unsigned long long, part, part);
    asm volatile("" : "+s"(ndir), "+s"(nbatch), "+s"(slice_len), "+s"(debug), "+s"(by_b.mul), "+s"(by_b.shift), "+s"(arrive_g), "+s"(stats_g),
                 NN_HELD(begin), NN_HELD(qblocks), "+s"(by_q_0.mul), "+s"(by_q_0.shift), "+s"(by_q_1.mul), "+s"(by_q_1.shift), NN_HELD(nq), NN_HELD(nt),
                 NN_HELD(slices), NN_HELD(ubegin), NN_HELD(q), NN_HELD(t), NN_HELD(out_d), NN_HELD(out_i), NN_HELD(part));
    int *const arrive = (int *)arrive_g;
    unsigned long long *const stats = (unsigned long long *)stats_g;
    const int d = (ndir > 1 && (int)blockIdx.x >= begin_1) ? 1 : 0;
    const int qblocks = NN_OF_DIR(qblocks), nq = NN_OF_DIR(nq), nt = NN_OF_DIR(nt), slices = NN_OF_DIR(slices), unit_begin = NN_OF_DIR(ubegin);
    const float *const q_dir = (const float *)NN_OF_DIR(q), *const t_dir = (const float *)NN_OF_DIR(t);
    float *const out_d_dir = (float *)NN_OF_DIR(out_d);
    int *const out_i_dir = (int *)NN_OF_DIR(out_i);
    unsigned long long *const part_dir = (unsigned long long *)NN_OF_DIR(part);
    // block id within the direction = (slice * b + batch) * qblocks + qblock
    const NNBlockId id = nn_decode_block((int)blockIdx.x - NN_OF_DIR(begin), qblocks, NNDiv{NN_OF_DIR(by_q).mul, NN_OF_DIR(by_q).shift}, nbatch, by_b);
    const int qb = id.qb, batch = id.batch, slice = id.slice;

    const float *__restrict__ Qp = q_dir + (size_t)batch * nq * 3;
    const float *__restrict__ T = t_dir + (size_t)batch * nt * 3;
    const float cx = NN_CONST(T)[0], cy = NN_CONST(T)[1], cz = NN_CONST(T)[2];

    const int k_begin = slice * slice_len;
    int k_end = k_begin + slice_len;
    if (k_end > nt) k_end = nt;

    float qx[Q], qy[Q], qz[Q], b0[Q], b1[Q], qq[Q];
    Top3 st[Q];
    const int q0 = (qb * kWavesPerBlock + wave) * (32 * Q) + col;
#pragma unroll
    for (int r = 0; r < Q; r++) {
        int j = q0 + r * 32;
        if (j >= nq) j = nq - 1;
        qx[r] = Qp[(size_t)j * 3 + 0];
        qy[r] = Qp[(size_t)j * 3 + 1];
        qz[r] = Qp[(size_t)j * 3 + 2];
        const float px = qx[r] - cx, py = qy[r] - cy, pz = qz[r] - cz;
        qq[r] = __fmaf_rn(pz, pz, __fmaf_rn(py, py, __fmul_rn(px, px)));
        b0[r] = half ? py : px;          // k = 0 (x) on lanes 0..31, k = 1 (y) on lanes 32..63
        b1[r] = half ? 1.0f : pz;        // k = 2 (z),               k = 3 (|t|^2 x 1)
        top3_init(st[r]);
    }

    f32x16 acc0[U * Q], acc1[U * Q];
    float2 A[U];
    auto fetch = [&](int rb) {
#pragma unroll
        for (int s = 0; s < U; s++) A[s] = plane[half][rb + s * 32 + col];
    };
    // MFMAs of the unit whose rows are in A, then the rows of unit `next` into A
    auto issue = [&](int next, f32x16 (&dst)[U * Q]) {
#pragma unroll
        for (int s = 0; s < U; s++) {
#pragma unroll
            for (int r = 0; r < Q; r++) {
                f32x16 c = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                c = __builtin_amdgcn_mfma_f32_32x32x2f32(A[s].x, b0[r], c, 0, 0, 0);
                dst[s * Q + r] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[s].y, b1[r], c, 0, 0, 0);
            }
        }
        fetch(next);
    };
    auto reduce = [&](const f32x16 (&src)[U * Q], int id) {
#pragma unroll
        for (int r = 0; r < Q; r++) {
            float m;
#pragma unroll
            for (int s = 0; s < U; s++) {
                const f32x16 &c = src[s * Q + r];
                // raw v_min3: fminf() would first canonicalise every MFMA output (v_max x,x)
                if (s == 0) asm("v_min3_f32 %0, %1, %2, %3" : "=v"(m) : "v"(c[0]), "v"(c[1]), "v"(c[2]));
                else        asm("v_min3_f32 %0, %1, %2, %3" : "=v"(m) : "v"(m), "v"(c[0]), "v"(c[1]));
#pragma unroll
                for (int i = (s == 0 ? 3 : 2); i + 1 < 16; i += 2)
                    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(m) : "v"(m), "v"(c[i]), "v"(c[i + 1]));
                if (s == 0) asm("v_min_f32 %0, %1, %2" : "=v"(m) : "v"(m), "v"(c[15]));
            }
            top3_insert(st[r], m, id);
        }
    };

    float tmax2 = 0.0f;
    float nf = 0.0f;      // NaN once a target of the slice had a non-finite coordinate
    for (int t0 = k_begin; t0 < k_end && !(debug & 4); t0 += kMTile) {
        const int tn = min(kMTile, k_end - t0);
        const int tn_pad = (tn + 2 * kC - 1) / (2 * kC) * (2 * kC);
        __syncthreads();
        for (int t = threadIdx.x; t < tn_pad; t += kBlock) {
            float ax = 0.0f, ay = 0.0f, az = 0.0f, tt = __builtin_inff();   // padding: +inf never wins
            if (t < tn) {
                const float *tp = T + (size_t)(t0 + t) * 3;
                const float x = tp[0] - cx, y = tp[1] - cy, z = tp[2] - cz;
                tt = __fmaf_rn(z, z, __fmaf_rn(y, y, __fmul_rn(x, x)));
                tmax2 = fmaxf(tmax2, tt);
                nf = __fmaf_rn(tt, 0.0f, nf);        // inf x 0 = NaN, NaN sticks (v_max drops NaNs)
                ax = -2.0f * x; ay = -2.0f * y; az = -2.0f * z;
            }
            plane[0][t] = make_float2(ax, az);
            plane[1][t] = make_float2(ay, tt);
        }
        __syncthreads();
        // Two-stage software pipeline over bookkeeping units: the MFMAs of unit i+1 are
        // issued before the VALU minima of unit i, into the other accumulator set.
        fetch(0);
        issue(kC, acc0);
        for (int rb = 0; rb < tn_pad; rb += 2 * kC) {
            issue(rb + 2 * kC, acc1);          // past the end: spare rows, results dropped
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_nop 7");           // a 16-pass MFMA result needs 19 wait states before the inline-asm
            reduce(acc0, t0 + rb);             // v_min3 (not padded by the compiler): 8 here + the instructions between
            __builtin_amdgcn_sched_barrier(0);
            issue(rb + 3 * kC, acc0);
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_nop 7");
            reduce(acc1, t0 + rb + kC);
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // lanes l and l^32 hold the two halves of the same queries: fold (both end up equal)
#pragma unroll
    for (int r = 0; r < Q; r++) {
        const float o1 = __shfl_xor(st[r].a1, 32), o2 = __shfl_xor(st[r].a2, 32), o3 = __shfl_xor(st[r].a3, 32);
        const int oc1 = __shfl_xor(st[r].c1, 32), oc2 = __shfl_xor(st[r].c2, 32);
        Top3 lo = st[r], hi = st[r];
        if (half) { lo.a1 = o1; lo.a2 = o2; lo.a3 = o3; lo.c1 = oc1; lo.c2 = oc2; }
        else      { hi.a1 = o1; hi.a2 = o2; hi.a3 = o3; hi.c1 = oc1; hi.c2 = oc2; }
        top3_insert(lo, hi.a1, hi.c1);
        top3_insert(lo, hi.a2, hi.c2);
        top3_insert(lo, hi.a3, -1);
        st[r] = lo;
    }
    // slice maximum of |t'|^2; +inf when a target is not finite: every query is then answered by
    // nn_exhaustive, which reproduces the reference's tile semantics for NaNs
    if (nf != nf) tmax2 = __builtin_inff();
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) tmax2 = fmaxf(tmax2, __shfl_xor(tmax2, o));
    __syncthreads();
    if (lane == 0) s_red[wave] = tmax2;
    __syncthreads();
    tmax2 = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));

    if (slices > 1) {
        // Per query and slice three 8-byte words (a1,c1) (a2,c2) (a3,tmax2), agent-scope
        // atomic stores / loads on both sides (see the VALU kernel); the last block to
        // arrive folds the slices in slice order.
        const size_t bnq = (size_t)nbatch * nq;
        unsigned long long *P = part_dir + (size_t)batch * nq;
        if (!half) {
#pragma unroll
            for (int r = 0; r < Q; r++) {
                const int j = q0 + r * 32;
                if (j < nq) {
                    unsigned long long *p = P + (size_t)slice * 3 * bnq + j;
                    __hip_atomic_store(p, ((unsigned long long)__float_as_uint(st[r].a1) << 32) | (unsigned)st[r].c1,
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(p + bnq, ((unsigned long long)__float_as_uint(st[r].a2) << 32) | (unsigned)st[r].c2,
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(p + 2 * bnq,
                                       ((unsigned long long)__float_as_uint(st[r].a3) << 32) | __float_as_uint(tmax2),
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        if (debug & 2) return;
        int *cnt = arrive + unit_begin + batch * qblocks + qb;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0)
            s_misc[0] = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (s_misc[0] != slices - 1) return;
        if (threadIdx.x == 0) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int r = 0; r < Q; r++) {
            int j = q0 + r * 32;
            j = j < nq ? j : nq - 1;
            Top3 f;
            top3_init(f);
            float tm = 0.0f;
            for (int s2 = 0; s2 < slices; s2++) {
                const unsigned long long *p = P + (size_t)s2 * 3 * bnq + j;
                const unsigned long long w0 = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned long long w1 = __hip_atomic_load(p + bnq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned long long w2 = __hip_atomic_load(p + 2 * bnq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                top3_insert(f, __uint_as_float((unsigned)(w0 >> 32)), (int)(unsigned)w0);
                top3_insert(f, __uint_as_float((unsigned)(w1 >> 32)), (int)(unsigned)w1);
                top3_insert(f, __uint_as_float((unsigned)(w2 >> 32)), -1);
                tm = fmaxf(tm, __uint_as_float((unsigned)w2));
            }
            st[r] = f;
            tmax2 = tm;      // the same for every query of the block
        }
    }

    // Decide, re-scan the listed tile(s) exactly, or flag the query for the exhaustive pass.
    float *__restrict__ od = out_d_dir + (size_t)batch * nq;
    int *__restrict__ oi = out_i_dir + (size_t)batch * nq;
    __syncthreads();
    if (threadIdx.x == 0) s_misc[1] = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < Q; r++) {
        const Top3 &f = st[r];
        bool two = false, flag = false;
        if (!nn_safe(f.a1, f.a2, qq[r], tmax2) || (debug & 16)) {
            two = true;
            if (!nn_safe(f.a1, f.a3, qq[r], tmax2) || f.c2 < 0) flag = true;
        }
        if (f.c1 < 0 || (debug & 8)) flag = true;
        if (!(tmax2 < __builtin_inff()) || !(qq[r] < __builtin_inff())) flag = true;      // non-finite input
        const int j = q0 + r * 32;
        if (flag) {
            if (!half && j < nq) s_flag[atomicAdd(&s_misc[1], 1)] = j;
            continue;
        }
        // lanes 0..31 take the first tile, lanes 32..63 the second (when needed and different)
        const int base = half ? f.c2 : f.c1;
        float bd = __builtin_inff();
        int bi = 0;
        if ((!half || (two && f.c2 != f.c1)) && !(debug & 1)) rescan_chunk<FMA, kC>(T, nt, base, qx[r], qy[r], qz[r], bd, bi);
        const float obd = __shfl_xor(bd, 32);
        const int obi = __shfl_xor(bi, 32);
        if (!half && j < nq) {
            const bool other = obd < bd || (obd == bd && obi < bi);
            od[j] = other ? obd : bd;
            oi[j] = other ? obi : bi;
        }
    }
    __syncthreads();
    const int nflag = s_misc[1];
    if (stats && threadIdx.x == 0) {
        atomicAdd(&stats[0], (unsigned long long)min(128 * Q, nq - qb * 128 * Q));
        atomicAdd(&stats[1], (unsigned long long)nflag);
    }
    for (int fidx = 0; fidx < nflag; fidx++) nn_exhaustive<FMA>(Qp, T, nt, s_flag[fidx], od, oi, s_red, s_fi);
}

// Chamfer backward, both directions in one launch (chamfer3D.cu:155-195).
// Thread j < B*N: direction 1 term of point j of cloud 1; B*N <= j < B*(N+M):
// direction 2 term of point j-B*N of cloud 2.  Accumulates with fp32 atomics
// into the caller-zeroed gradients, exactly like the reference.  Small calls: one launch is what a call costs (large
// calls take chamfer_grad_dir_kernel below: the atomics, six per point at ~14 per clock chip-wide, bound this kernel).
__global__ __launch_bounds__(kBlock) void chamfer_grad_kernel(int b, int n, const float *__restrict__ xyz1, int m,
                                                              const float *__restrict__ xyz2,
                                                              const float *__restrict__ gd1, const int *__restrict__ idx1,
                                                              const float *__restrict__ gd2, const int *__restrict__ idx2,
                                                              float *__restrict__ gx1, float *__restrict__ gx2)
{
    long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    const long long bn = (long long)b * n, bm = (long long)b * m;
    const float *P1, *P2, *G;
    const int *I;
    float *O1, *O2;
    int np1, np2;
    if (t < bn) {
        P1 = xyz1; P2 = xyz2; G = gd1; I = idx1; O1 = gx1; O2 = gx2; np1 = n; np2 = m;
    } else if (t < bn + bm) {
        t -= bn;
        P1 = xyz2; P2 = xyz1; G = gd2; I = idx2; O1 = gx2; O2 = gx1; np1 = m; np2 = n;
    } else {
        return;
    }
    const long long i = t / np1;
    const float x1 = P1[t * 3 + 0], y1 = P1[t * 3 + 1], z1 = P1[t * 3 + 2];
    const long long j2 = i * np2 + I[t];
    const float x2 = P2[j2 * 3 + 0], y2 = P2[j2 * 3 + 1], z2 = P2[j2 * 3 + 2];
    const float g = __fmul_rn(G[t], 2.0f);
    const float vx = __fmul_rn(g, x1 - x2), vy = __fmul_rn(g, y1 - y2), vz = __fmul_rn(g, z1 - z2);
    atomicAdd(&O1[t * 3 + 0], vx);
    atomicAdd(&O1[t * 3 + 1], vy);
    atomicAdd(&O1[t * 3 + 2], vz);
    atomicAdd(&O2[j2 * 3 + 0], -vx);
    atomicAdd(&O2[j2 * 3 + 1], -vy);
    atomicAdd(&O2[j2 * 3 + 2], -vz);
}

constexpr int kGradBlock = 1024;      // (64 x 32768 both ways: 122 us; 512 threads 144, 256 threads 228 before the loads were batched; capped at 64 VGPRs for two blocks per CU 159)

// Large calls, round 6: ONE pass per direction computes every term once and puts it in both places (chamfer3D.cu:157-171) --
// a block owns a tile of kGradTile target rows of one cloud; it walks the other cloud's index array, and for the entries that
// land in its tile (exactly one block per entry) it evaluates the term, adds it to the QUERY's own gradient row (a plain
// read-modify-write: that row has no other writer in this launch) and accumulates its negative in the tile's LDS copy, which
// is added to the gradient at the end (a plain coalesced read-modify-write: the tile has one owner).  Direction 0 and
// direction 1 are two launches (each cloud's gradient is "own rows" in one and "tiles" in the other).  Against round 5's
// own-row launch + tile launch: the rows, weights and indices are read once, not twice; the hits of a wave's 512 entries are
// compacted so that only they issue loads (round 5 loaded for all eight entries of a thread at clamped addresses: seven of
// eight load instructions fetched nothing); the blocks of a batch element share an XCD, so the tiles' walks of the same index
// array and the partial lines of the own rows meet in one L2.
constexpr int kGradList = 128;     // compacted hits a wave keeps per trip (more: the hits are dense, the lanes take them in place)
constexpr int kGradTile = 4096;    // target rows a block owns
__global__ __launch_bounds__(kGradBlock) void chamfer_grad_dir_kernel(int b, int tiles, int nq, const float *__restrict__ Qc, int nt,
                                                                      const float *__restrict__ Tc, const float *__restrict__ Gd,
                                                                      const int *__restrict__ Ix, float *__restrict__ Oq,
                                                                      float *__restrict__ Ot)
{
    __shared__ float acc[kGradTile * 3];
    __shared__ unsigned long long lst[kGradBlock / kWave][kGradList];      // query << 32 | row of the tile
    int e, tile;
    {
        const int lin = blockIdx.x;
        if ((b & 7) == 0) { const int xcd = lin & 7, k = lin >> 3; e = 8 * (k / tiles) + xcd; tile = k % tiles; }
        else { e = lin / tiles; tile = lin % tiles; }
    }
    if (e >= b) return;
    const int t0 = tile * kGradTile;
    const float *__restrict__ Q = Qc + (size_t)e * nq * 3;
    const float *__restrict__ T = Tc + (size_t)e * nt * 3;
    const float *__restrict__ G = Gd + (size_t)e * nq;
    const int *__restrict__ I = Ix + (size_t)e * nq;
    float *__restrict__ OQ = Oq + (size_t)e * nq * 3;
    float *__restrict__ OT = Ot + (size_t)e * nt * 3;
    const int rows = min(kGradTile, nt - t0);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < rows * 3; i += kGradBlock) acc[i] = 0.0f;
    __syncthreads();
    auto term = [&](int q, int k) {
        const float qx = Q[(size_t)q * 3 + 0], qy = Q[(size_t)q * 3 + 1], qz = Q[(size_t)q * 3 + 2];
        const float g = __fmul_rn(G[q], 2.0f);
        const float tx = T[(size_t)(t0 + k) * 3 + 0], ty = T[(size_t)(t0 + k) * 3 + 1], tz = T[(size_t)(t0 + k) * 3 + 2];
        const float o0 = OQ[(size_t)q * 3 + 0], o1 = OQ[(size_t)q * 3 + 1], o2 = OQ[(size_t)q * 3 + 2];
        const float vx = __fmul_rn(g, qx - tx), vy = __fmul_rn(g, qy - ty), vz = __fmul_rn(g, qz - tz);
        OQ[(size_t)q * 3 + 0] = __fadd_rn(o0, vx);
        OQ[(size_t)q * 3 + 1] = __fadd_rn(o1, vy);
        OQ[(size_t)q * 3 + 2] = __fadd_rn(o2, vz);
        atomicAdd(&acc[k * 3 + 0], -vx);
        atomicAdd(&acc[k * 3 + 1], -vy);
        atomicAdd(&acc[k * 3 + 2], -vz);
    };
    for (int q0 = threadIdx.x; q0 - (int)threadIdx.x < nq; q0 += 8 * kGradBlock) {      // (wave-uniform trip count)
        int kk[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int q = q0 + u * kGradBlock;
            kk[u] = q < nq ? I[q] - t0 : -1;
        }
        // the wave's hits among its 512 entries
        int pos[8], total = 0;
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const bool hit = (unsigned)kk[u] < (unsigned)rows;
            const unsigned long long m = __ballot(hit);
            pos[u] = hit ? total + (int)__popcll(m & ((1ull << lane) - 1ull)) : -1;
            total += (int)__popcll(m);
        }
        if (total == 0) continue;
        if (total <= kGradList) {
#pragma unroll
            for (int u = 0; u < 8; u++)
                if (pos[u] >= 0) lst[wave][pos[u]] = ((unsigned long long)(unsigned)(q0 + u * kGradBlock) << 32) | (unsigned)kk[u];
            // (the list is this wave's own: LDS operations of a wave are performed in order)
            for (int i = lane; i < total; i += kWave) {
                const unsigned long long w = lst[wave][i];
                term((int)(w >> 32), (int)(unsigned)w);
            }
        } else {
#pragma unroll
            for (int u = 0; u < 8; u++)
                if (pos[u] >= 0) term(q0 + u * kGradBlock, kk[u]);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < rows * 3; i += kGradBlock) OT[(size_t)t0 * 3 + i] = __fadd_rn(OT[(size_t)t0 * 3 + i], acc[i]);
}

struct NNConfig {
    int family;           // GENPC_NN_PATH: 4 cell-sorted pruned search (opt-in: wins when most queries have a near target), 3 two-piece f16 MFMA filter (default), 1 fp32 MFMA filter (small problems), 0 VALU path (cross-check); -1: not given
    int r, q, u, wps;     // GENPC_NN_R / _Q / _U / _WPS as given: nn_plan.h says which values count
    int dbg;              // GENPC_NN_DEBUG
};

// genpc_nn_tune() overrides (-1: use the environment / default).  Thread-local: a test that
// switches kernel families does not change what other host threads launch.
thread_local int t_tune_path = -1, t_tune_hooks = -1;      // (declared in common.h: genpc_thread_state_export / _import)

// Tunables; the environment is read ONCE, at first use (C++11 static initialisation is
// thread-safe), never per launch.
static const NNConfig &nn_config()
{
    static const NNConfig c = [] {
        NNConfig k{-1, 0, 0, 0, 0, 0};
        k.r = tune_env("GENPC_NN_R", 0, "VALU nearest-neighbour path: queries per lane (2 | 4, 0 = pick)");
        if (const char *e = tune_env_str("GENPC_NN_PATH", "nearest-neighbour kernel family: valu | mfma32 | f16 (default) | grid (opt-in)")) {
            if (e[0] == 'v') k.family = kNNValu;
            else if (e[0] == 'm') k.family = kNNMfma32;
            else if (e[0] == 'f') k.family = kNNF16;
            else if (e[0] == 'g') k.family = kNNGrid;
            else fprintf(stderr, "genpc_hip: GENPC_NN_PATH=%s is not one of valu | mfma32 | f16 | grid: keeping the default (f16)\n", e);
        }
        k.q = tune_env("GENPC_NN_Q", 0, "MFMA filter: 32-query tiles per wave (2 | 4, 0 = pick)");
        k.u = tune_env("GENPC_NN_U", 0, "MFMA filter: target tiles per bookkeeping unit (2 | 4, 0 = pick)");
        k.wps = tune_env("GENPC_NN_WPS", 0, "resident blocks per CU the nearest-neighbour planner assumes (0 = per kernel family)");
        k.dbg = tune_env("GENPC_NN_DEBUG", 0, "test hooks of the filtered nearest-neighbour paths (bit mask, see genpc_nn_tune)");
        return k;
    }();
    return c;
}

// What nn_plan may depend on beside the sizes: the device, the calling thread's family, the switches.
static NNAsk nn_ask(int b, int cus)
{
    const NNConfig &cfg = nn_config();
    NNAsk ask;
    ask.b = b;
    ask.cus = cus > 0 ? cus : num_cus();
    ask.forced = t_tune_path;
    ask.env_family = cfg.family;
    ask.env_r = cfg.r;
    ask.env_q = cfg.q;
    ask.env_u = cfg.u;
    ask.env_wps = cfg.wps;
    return ask;
}

template <int Q, int U>
static void launch_mfma(const NNArgs &a, int blocks, hipStream_t st)
{
    if (a.fma)
        hipLaunchKernelGGL((nn_mfma_kernel<Q, U, 1>), dim3(blocks), dim3(kBlock), 0, st, a);
    else
        hipLaunchKernelGGL((nn_mfma_kernel<Q, U, 0>), dim3(blocks), dim3(kBlock), 0, st, a);
}

template <int R>
static void launch_r(const NNArgs &a, int blocks, hipStream_t st)
{
    if (a.fma)
        hipLaunchKernelGGL((nn_forward_kernel<R, 1>), dim3(blocks), dim3(kBlock), 0, st, a);
    else
        hipLaunchKernelGGL((nn_forward_kernel<R, 0>), dim3(blocks), dim3(kBlock), 0, st, a);
}

// Duplicate pre-pass policy of the f16 filter (nn_dedupe.hip).  The pre-pass is two launches with three dependent
// memory round trips each: 26 us on an idle GPU whatever the size, 59 us at 8 x 32768 x 2 points -- against 33 us for
// the whole headline step.  So it runs
//   * when the caller brings the masks (the alignment loop, ICP and the scale search make them once per call: their
//     clouds' duplicates are the same at every step / for every candidate), or
//   * while the input asks for it.  The finish kernel adds (a sample of) the queries it had to re-do exhaustively to
//     a host-visible word, the pre-pass adds (a sample of) the copies it found to another; the NEXT call reads both:
//     many re-dos switch the pre-pass on, a pre-pass that finds next to nothing switches it off again.  The words are
//     read without any synchronisation -- a stale value delays the switch by a call; results do not depend on it (the
//     masks only remove targets that can never be reported).
// Hooks 2048 / 4096 of genpc_nn_tune force it off / on (tests).
struct DedupeHint {
    unsigned *host = nullptr;          // cumulative, written by the GPU: [0] exhaustive re-dos, [1] copies found, [2] pre-passes completed (hipHostMalloc, mapped)
    std::mutex mu;
    unsigned seen[3] = {0, 0, 0};      // what the host has accounted for
    bool on = false;
};
static DedupeHint *dedupe_hint()
{
    static DedupeHint hints[16];
    static std::mutex mu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
    DedupeHint &h = hints[dev];
    if (!h.host) {
        std::lock_guard<std::mutex> l(mu);
        if (!h.host) {
            void *p = nullptr;
            if (hipHostMalloc(&p, 64, hipHostMallocMapped) != hipSuccess) return nullptr;
            for (int i = 0; i < 16; i++) ((volatile unsigned *)p)[i] = 0;
            h.host = (unsigned *)p;
        }
    }
    return &h;
}

int nn_forward(int b, int ndir, const float *q0, int n0, const float *t0, int m0, float *d0, int *i0,
               const float *q1, int n1, const float *t1, int m1, float *d1, int *i1, hipStream_t st,
               float radius2, const unsigned *dup0, const unsigned *dup1, int dup_shared)
{
    NNArgs a{};
    a.b = b;
    a.fma = arith_mode() != 0 ? 1 : 0;
    a.radius2 = radius2;
    a.debug = t_tune_hooks >= 0 ? t_tune_hooks : nn_config().dbg;
    if (a.debug & 512) {
        a.stats = (unsigned long long *)workspace(kWsNnStats, 256, nullptr, nullptr, 256);      // one block per device, shared by all streams
        if (!a.stats) return 0;
    }
    const float *qs[2] = {q0, q1};
    const float *ts[2] = {t0, t1};
    float *ds[2] = {d0, d1};
    int *is[2] = {i0, i1};
    const unsigned *dups[2] = {dup0, dup1};
    const int nqs[2] = {n0, n1}, nts[2] = {m0, m1};
    NNAsk ask = nn_ask(b, 0);
    for (int d = 0; d < ndir; d++) {
        if (!ask.add(nqs[d], nts[d])) continue;
        NNDir &D = a.dir[ask.ndir - 1];
        D.q = qs[d]; D.t = ts[d]; D.out_d = ds[d]; D.out_i = is[d];
        D.nq = nqs[d]; D.nt = nts[d];
        D.dupmask = dups[d];
        D.dup_shared = dups[d] ? dup_shared : 0;
    }
    const int nd = a.ndir = ask.ndir;
    if (nd == 0) return 1;
    ask.swapped = nd == 2 && a.dir[1].q == a.dir[0].t && a.dir[1].t == a.dir[0].q;
    ask.radius = radius2 < __builtin_inff();

    const NNPlan plan = nn_plan(ask);
    if (plan.family == kNNGrid) return launch_nn_grid(a, st);
    if (plan.too_large) {
        set_error("chamfer: problem too large for one launch");
        return 0;
    }
    a.slice_len = plan.slice_len;
    a.hint_stride = plan.hint_stride;
    a.by_b = nn_div_make(b);
    bool any_partials = false;
    for (int d = 0; d < nd; d++) {
        NNDir &D = a.dir[d];
        const NNPlanDir &P = plan.dir[d];
        D.qblocks = P.qblocks;
        D.by_qblocks = nn_div_make(P.qblocks);
        D.slices = D.ntmax = P.slices;      // (ntmax: the f16 filter keeps one maximum per slice)
        D.block_begin = P.block_begin;
        D.unit_begin = P.unit_begin;
        D.fin_begin = P.fin_begin;
        any_partials = any_partials || P.partials;
    }
    if (any_partials) {
        // [arrival counters | per-slice partials]; counters are zeroed when the block is
        // (re)allocated and restored to zero by the merging block, so steady-state calls
        // need no memset.
        // Usually the counters fit the 64 KiB prefix that is zero between calls.  A launch with more
        // query blocks than that (1000 scale-search candidates x 128 blocks) takes a larger area,
        // which earlier calls used for partials: it is cleared on the stream first (the kernels hand
        // every counter back as zero, so the 64 KiB invariant survives such a call).
        const size_t cnt_min = (size_t)1 << 16;
        const size_t cnt_ints = std::max(cnt_min / sizeof(int), (size_t)plan.units);
        unsigned long long *wp;
        WsLayout L;
        L.add(a.arrive, cnt_ints);
        L.add_tail(wp, (size_t)plan.part_words);          // (both directions' partials, handed out below)
        if (!ws_alloc(L, kWsNnForward, st, nullptr, cnt_min)) return 0;
        if (cnt_ints * sizeof(int) > cnt_min && !check(hipMemsetAsync(a.arrive, 0, (char *)wp - (char *)a.arrive, st), "hipMemsetAsync(arrival counters)")) return 0;
        size_t off = 0;
        for (int d = 0; d < nd; d++) {
            if (!plan.dir[d].partials) continue;
            a.dir[d].part = wp + off;
            off += (size_t)a.dir[d].slices * b * a.dir[d].nq * plan.pwords;
        }
    }
    if (plan.family == kNNF16) {
        // exact duplicates among the targets (policy above nn_forward)
        const int force = (a.debug & 2048) ? 0 : ((a.debug & 4096) ? 1 : -1);
        DedupeHint *H = dedupe_hint();
        bool own_masks = true;
        for (int d = 0; d < nd; d++) own_masks = own_masks && a.dir[d].dupmask != nullptr;
        if (force == 0) {
            for (int d = 0; d < nd; d++) a.dir[d].dupmask = nullptr;
        } else if (!own_masks) {
            long long queries = 0, targets = 0;
            for (int d = 0; d < nd; d++) { queries += (long long)b * a.dir[d].nq; targets += (long long)b * a.dir[d].nt; }
            bool run = force == 1;
            if (!run && H) {
                // Evidence the GPU has delivered since the last look (cumulative words: a host that runs ahead of the
                // GPU simply sees no news and keeps its state): re-dos of calls that ran without the pre-pass switch
                // it on, completed pre-passes that found next to nothing switch it off.
                std::lock_guard<std::mutex> l(H->mu);
                volatile unsigned *hv = H->host;
                const unsigned redo = hv[0] - H->seen[0], found = hv[1] - H->seen[1], done = hv[2] - H->seen[2];
                H->seen[0] += redo; H->seen[1] += found; H->seen[2] += done;
                if (!H->on) {
                    if ((long long)redo * 32 > queries) H->on = true;
                } else if (done > 0 && (long long)(found / done) * 32 < targets) {
                    H->on = false;
                }
                run = H->on;
            }
            if (run) {
                // one pre-pass per distinct target cloud (the two directions' targets are each other's queries)
                const float *pp[2];
                int pn[2];
                unsigned *pm[2];
                size_t words[2];
                int nc = 0;
                for (int d = 0; d < nd; d++) {
                    pp[nc] = a.dir[d].t;
                    pn[nc] = a.dir[d].nt;
                    words[nc] = (nn_dedupe_mask_words(b, pn[nc]) + 63) & ~(size_t)63;
                    nc++;
                }
                unsigned *mw = (unsigned *)workspace(kWsNnDupMasks, (words[0] + (nc > 1 ? words[1] : 0)) * sizeof(unsigned), st);
                if (!mw) return 0;
                pm[0] = mw;
                pm[1] = mw + words[0];
                if (!launch_nn_dedupe(b, nc, pp, pn, pm, H ? H->host + 1 : nullptr, st)) return 0;
                for (int d = 0; d < nd; d++) { a.dir[d].dupmask = pm[d]; a.dir[d].dup_shared = 0; }
            }
        }
        a.hint = H ? H->host : nullptr;
        return launch_nn_f16(a, plan, st);
    }
    const int blocks = (int)plan.blocks;
    if (plan.family == kNNMfma32) {
        if (plan.q == 2) { if (plan.unit == 2) launch_mfma<2, 2>(a, blocks, st); else launch_mfma<2, 1>(a, blocks, st); }
        else             { if (plan.unit == 2) launch_mfma<1, 2>(a, blocks, st); else launch_mfma<1, 1>(a, blocks, st); }
    } else if (plan.r == 4) {
        launch_r<4>(a, blocks, st);
    } else {
        launch_r<2>(a, blocks, st);
    }
    return check(hipGetLastError(), "nn_forward_kernel launch") ? 1 : 0;
}

}  // namespace genpc

GENPC_API int genpc_nn_tune(int path, int hooks)
{
    const int env = genpc::nn_config().family;
    const int prev = genpc::t_tune_path >= 0 ? genpc::t_tune_path : (env >= 0 ? env : (int)genpc::kNNF16);
    if (path == genpc::kNNValu || path == genpc::kNNMfma32 || path == genpc::kNNF16 || path == genpc::kNNGrid) genpc::t_tune_path = path;
    if (hooks >= 0) genpc::t_tune_hooks = hooks;
    return prev;
}

GENPC_API int genpc_nn_plan(int b, int n, int m, int ndir, int cus, int out[16])
{
    using namespace genpc;
    if (!out || ndir < 1 || ndir > 2) return -1;
    // the shape as genpc_chamfer_forward (ndir 2) / genpc_nm_distance (ndir 1) bring it
    NNAsk ask = nn_ask(b, cus);
    ask.add(n, m);
    if (ndir == 2) ask.add(m, n);
    ask.swapped = ask.ndir == 2;
    const NNPlan p = nn_plan(ask);
    const int v[16] = {p.family, p.form, p.family == kNNValu ? p.r : p.q, p.unit, p.nl, p.slice_len, p.dir[0].slices, p.dir[1].slices,
                       (int)std::min<long long>(p.blocks, 0x7fffffff), (int)std::min<long long>(p.fin_blocks, 0x7fffffff), p.early, p.too_large,
                       p.dir[0].qblocks, p.dir[1].qblocks, p.hint_stride, ask.cus};
    for (int i = 0; i < 16; i++) out[i] = v[i];
    return 1;
}

GENPC_API int genpc_nn_stats(unsigned long long out[3], int reset, void *stream)
{
    using namespace genpc;
    unsigned long long *dev = (unsigned long long *)workspace(kWsNnStats, 256, nullptr, nullptr, 256);
    if (!dev) return 0;
    if (!check(hipStreamSynchronize((hipStream_t)stream), "genpc_nn_stats sync")) return 0;
    if (!check(hipMemcpy(out, dev, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost), "genpc_nn_stats copy")) return 0;
    if (reset && !check(hipMemset(dev, 0, 256), "genpc_nn_stats reset")) return 0;
    return 1;
}

GENPC_API int genpc_chamfer_forward(int b, int n, const float *xyz1, int m, const float *xyz2, float *dist1,
                                    int *idx1, float *dist2, int *idx2, void *stream)
{
    return genpc::nn_forward(b, 2, xyz1, n, xyz2, m, dist1, idx1, xyz2, m, xyz1, n, dist2, idx2,
                             (hipStream_t)stream);
}

GENPC_API int genpc_nm_distance(int b, int n, const float *xyz, int m, const float *xyz2, float *result,
                                int *result_i, void *stream)
{
    return genpc::nn_forward(b, 1, xyz, n, xyz2, m, result, result_i, nullptr, 0, nullptr, 0, nullptr, nullptr,
                             (hipStream_t)stream);
}

GENPC_API int genpc_nm_distance_within(int b, int n, const float *xyz, int m, const float *xyz2, float radius2,
                                       float *result, int *result_i, void *stream)
{
    if (!(radius2 >= 0.0f)) {
        genpc::set_error("genpc_nm_distance_within: radius2 must be >= 0");
        return -1;
    }
    return genpc::nn_forward(b, 1, xyz, n, xyz2, m, result, result_i, nullptr, 0, nullptr, 0, nullptr, nullptr,
                             (hipStream_t)stream, radius2);
}

GENPC_API int genpc_chamfer_backward(int b, int n, const float *xyz1, int m, const float *xyz2,
                                     const float *graddist1, const int *idx1, const float *graddist2,
                                     const int *idx2, float *gradxyz1, float *gradxyz2, void *stream)
{
    using namespace genpc;
    // The reference indexes xyz2 with idx1 unconditionally; with an empty cloud
    // there is nothing to differentiate.
    if (b <= 0 || n <= 0 || m <= 0) return 1;
    long long total = (long long)b * n + (long long)b * m;
    long long blocks = ceil_div64(total, kBlock);
    if (blocks > 0x7fffffffLL) {
        set_error("chamfer backward: problem too large for one launch");
        return 0;
    }
    // from 262144 points (both clouds) the gradient is accumulated through LDS tiles that own their output rows instead of
    // global atomics
    if ((long long)b * ((long long)n + m) >= 262144) {
        const int tiles_n = ceil_div(n, kGradTile), tiles_m = ceil_div(m, kGradTile);
        // (a grid of more than 2^31 blocks -- no call fits such clouds in memory -- takes the atomics below)
        if ((long long)b * (tiles_n > tiles_m ? tiles_n : tiles_m) <= 0x7fffffffLL) {
            // direction 0: queries = cloud 1, tiles of cloud 2's gradient; direction 1 the converse
            hipLaunchKernelGGL(chamfer_grad_dir_kernel, dim3((unsigned)(b * tiles_m)), dim3(kGradBlock), 0, (hipStream_t)stream, b, tiles_m,
                               n, xyz1, m, xyz2, graddist1, idx1, gradxyz1, gradxyz2);
            hipLaunchKernelGGL(chamfer_grad_dir_kernel, dim3((unsigned)(b * tiles_n)), dim3(kGradBlock), 0, (hipStream_t)stream, b, tiles_n,
                               m, xyz2, n, xyz1, graddist2, idx2, gradxyz2, gradxyz1);
            return check(hipGetLastError(), "chamfer_grad_dir_kernel launch") ? 1 : 0;
        }
    }
    hipLaunchKernelGGL(chamfer_grad_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, b, n, xyz1, m,
                       xyz2, graddist1, idx1, graddist2, idx2, gradxyz1, gradxyz2);
    return check(hipGetLastError(), "chamfer_grad_kernel launch") ? 1 : 0;
}
