// emd_steps.h -- the steps of one auction round on ONE cloud, stated once for the launch-per-round kernels of emd.hip (a cloud
// is a batch element) and of emd_ragged.hip (a cloud is a pair): the tiled bid over all objects -- staging, filter scan, lane
// merge, tie re-scan, the bid's four words --, GetMax's election and Assign's three cases per bidder, the single-workgroup
// resolve, and CalcDist / the gradient per point.  A kernel builds a view of its cloud (every pointer already at the cloud's
// own piece) and keeps what only it has around the calls.  All of it is inlined: the views never exist in memory.
#pragma once
#include "emd.h"

namespace genpc {

// ---------------- the tiled bid (emd_cuda.cu:95-179) ----------------
struct EmdBidCloud {
    int n, U;                          // objects (= points), bidders this round
    float eps;
    const float *X2, *PR;              // objects [n,3] and their prices
    int *bid, *second;                 // per point: the object it bid for and its second-best (the next bid's filter seeds)
    float *bid_increments, *max_increments;
};

// one tile of objects as four planes (x, y, z, price): a 16-byte read delivers four consecutive objects' x as two register
// pairs for the packed fp32 filter below
template <int TILE>
struct __attribute__((aligned(16))) BidTile { float x[TILE], y[TILE], z[TILE], p[TILE]; };

// a bidder as its lanes see it: the point and the filter's seed (by value: nothing below changes them) ...
struct BidPoint { float x1, y1, z1, seed; };
// ... and what a lane carries through the scan: the filter's threshold and the lane's own top-2
struct BidLane {
    float cb, best, better;
    int best_i, better_i;
};

__device__ __forceinline__ BidLane bid_lane(float seed)
{
    BidLane b;
    b.best = b.better = -1e9f;
    b.best_i = b.better_i = -1;
    b.cb = filter_cb(fmaxf(b.better, seed));
    return b;
}

// this thread's objects of the tile at k2, into registers (a tile is staged from them one or more tiles later)
template <int TILE>
__device__ __forceinline__ void bid_fetch(float4 (&pre)[TILE / 256], const EmdBidCloud &c, int k2)
{
#pragma unroll
    for (int i = 0; i < TILE / 256; i++) {
        const int k = k2 + threadIdx.x + i * kEBlock;
        const int kk = k < c.n ? k : c.n - 1;
        pre[i] = make_float4(c.X2[(size_t)kk * 3 + 0], c.X2[(size_t)kk * 3 + 1], c.X2[(size_t)kk * 3 + 2], c.PR[kk]);
    }
}

// Stages the tile at k2 from `pre`, requests the tile at k_next into the same registers (if below k_hi) and scans the
// staged one: lane p of P visits four consecutive objects per trip.  All threads of the workgroup call it together.
template <int FMA, int TILE>
__device__ __forceinline__ void bid_tile_step(BidTile<TILE> &s, float4 (&pre)[TILE / 256], const EmdBidCloud &c, const BidPoint pt, BidLane &b, int p, int P,
                                              int k2, int k_next, int k_hi)
{
    const int end_k = min(c.n, k2 + TILE) - k2;
    __syncthreads();                               // the previous tile has been scanned
#pragma unroll
    for (int i = 0; i < TILE / 256; i++) {
        const int t = threadIdx.x + i * kEBlock;
        if (t < end_k) { s.x[t] = pre[i].x; s.y[t] = pre[i].y; s.z[t] = pre[i].z; s.p[t] = pre[i].w; }
    }
    __syncthreads();
    if (k_next < k_hi) bid_fetch<TILE>(pre, c, k_next);
    // Pre-filter.  A candidate can change this lane's (best, better) only if its
    // value exceeds `better`, i.e. only if sqrt(s) < 3 - price - better.  That is
    // tested conservatively in squared space with fp32 and no sqrt / fp64:
    // cb = (3 - better) + 2e-6 (1 + |better|) absorbs every rounding of the test itself at
    // ANY magnitude of the clouds (filter_cb: the slack needed is u (21 + 9 |better|),
    // u = 2^-24, the slack given 33 u (1 + |better|)), so a candidate that fails the
    // test provably evaluates to d <= better and the exact update would be a
    // no-op.  The exact path (double-precision expression of emd_cuda.cu:146)
    // runs for the whole wave when any lane passes; for lanes that did not pass
    // it is that same no-op.  Results are therefore bit-identical with and
    // without the filter.
    // Four CONSECUTIVE objects per lane and iteration (4*P divides every tile length: n % 256 == 0,
    // P <= 64), evaluated two per instruction (packed fp32: same operations, same roundings as
    // sqdist and filter_cb's test); a lane's verdicts stay in SGPRs (one ballot per object), so a
    // group none of whose members can matter costs 16 packed operations, 4 compares and one scalar branch
    // (28 instead of 51 instructions per four objects; in-run A/B with the 1024-object tiles: 13 x 16384 7.68 ->
    // 7.31 ms, 8 x 32768 16.05 -> 15.05 -- with 2048-object tiles and half the resident waves it LOST 6 %;
    // issuing the next group's LDS reads early costs registers and residency: 7.23 -> 8.6 ms).
    const v2f x1v = {pt.x1, pt.x1}, y1v = {pt.y1, pt.y1}, z1v = {pt.z1, pt.z1};
    for (int t = 4 * p; t < end_k; t += 4 * P) {
        const float4 X4 = *(const float4 *)&s.x[t], Y4 = *(const float4 *)&s.y[t], Z4 = *(const float4 *)&s.z[t],
                     W4 = *(const float4 *)&s.p[t];
        const v2f cbv = {b.cb, b.cb};
        v2f sqv[2];
        unsigned long long pass[4];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const v2f dx = (h ? (v2f){X4.z, X4.w} : (v2f){X4.x, X4.y}) - x1v;
            const v2f dy = (h ? (v2f){Y4.z, Y4.w} : (v2f){Y4.x, Y4.y}) - y1v;
            const v2f dz = (h ? (v2f){Z4.z, Z4.w} : (v2f){Z4.x, Z4.y}) - z1v;
            if (FMA) sqv[h] = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dx, dx, dy * dy));
            else sqv[h] = (dx * dx + dy * dy) + dz * dz;
            const v2f tt = cbv - (h ? (v2f){W4.z, W4.w} : (v2f){W4.x, W4.y});
            const v2f t2 = tt * tt;
            pass[2 * h] = __ballot(sqv[h].x < t2.x);
            pass[2 * h + 1] = __ballot(sqv[h].y < t2.y);
        }
        if ((pass[0] | pass[1] | pass[2] | pass[3]) != 0ull) {
            const float sq[4] = {sqv[0].x, sqv[0].y, sqv[1].x, sqv[1].y};
            const float pr[4] = {W4.x, W4.y, W4.z, W4.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (pass[i] != 0ull) {
                    const float r = sqrtf(sq[i]);
                    const float d = (float)((3.0 - (double)r) - (double)pr[i]);
                    insert_top2(b.best, b.better, b.best_i, b.better_i, d, k2 + t + i);
                }
            }
            b.cb = filter_cb(fmaxf(b.better, pt.seed));
        }
    }
}

// merges the P partial top-2s of a bidder (value-symmetric): every lane of the bidder ends with the same four words
__device__ __forceinline__ void bid_merge_lanes(BidLane &b, int P)
{
    for (int off = 1; off < P; off <<= 1) {
        const float ob = __shfl_xor(b.best, off, kWave);
        const float obb = __shfl_xor(b.better, off, kWave);
        const int oi = __shfl_xor(b.best_i, off, kWave);
        const int obi = __shfl_xor(b.better_i, off, kWave);
        merge_top2(b.best, b.better, b.best_i, b.better_i, ob, obb, oi, obi);
    }
}

// Exact tie for first place: the bidder's P lanes re-scan ALL objects and pick the tied one the reference's scan meets
// first.  A bidder nothing ties with (it has no candidate at all: its coordinates are not finite) gets object -1.
template <int FMA>
__device__ __forceinline__ void bid_break_tie(const EmdBidCloud &c, const BidPoint pt, BidLane &b, bool active, int p, int P)
{
    const bool tie = active && (b.best == b.better);
    if (!__any(tie)) return;
    unsigned long long key = ~0ull;
    if (tie) {
        const int thread_per_unass = ref_thread_per_unass(c.n, c.U);
        for (int k = p; k < c.n; k += P) {
            const float d = bid_value<FMA>(pt.x1, pt.y1, pt.z1, c.X2[(size_t)k * 3 + 0], c.X2[(size_t)k * 3 + 1], c.X2[(size_t)k * 3 + 2], c.PR[k]);
            if (d == b.best) {
                const unsigned long long kk = ref_tie_key(k, c.n, thread_per_unass);
                key = kk < key ? kk : key;
            }
        }
    }
    for (int off = 1; off < P; off <<= 1) {
        const unsigned long long o = __shfl_xor(key, off, kWave);
        key = o < key ? o : key;
    }
    if (tie) b.best_i = (int)(key & 0xffffffffu);
}

// The bid of point j, by one lane of the bidder: returns the increment and the object bid for.  CLAMPED (the ragged call):
// the seeds are always kept, and a bid on "object -1" (bid_break_tie) becomes one on object 0 of the cloud; otherwise the
// reference's behaviour stands.
template <bool CLAMPED>
__device__ __forceinline__ float bid_write(const EmdBidCloud &c, const BidLane &b, int j, int &object)
{
    const float inc = __fadd_rn(__fsub_rn(b.best, b.better), c.eps);
    object = CLAMPED && (unsigned)b.best_i >= (unsigned)c.n ? 0 : b.best_i;
    c.bid[j] = object;
    if (CLAMPED || c.second != nullptr) c.second[j] = b.better_i;
    c.bid_increments[j] = inc;
    atomic_max_float(&c.max_increments[object], inc);
    return inc;
}

// ---------------- GetMax and Assign (emd_cuda.cu:181-215) ----------------
struct EmdRoundCloud {
    const int *list;                   // this round's bidders
    int *list_next, *cnt_next;         // next round's: losers and evicted owners; cnt_next is the cloud's own counter
    int *assignment, *assignment_inv, *max_idx;
    const int *bid;
    const float *bid_increments;
    float *price, *max_increments;
    const int *pos_of;                 // with price_s: the object's place in the cell-sorted copy (emd_grid.hip), whose price
    float *price_s;                    // is kept in step at price_s[4 * pos_of[object]]; null where there is no such copy
};

// GetMax.  In the forced last round every bidder is "assigned", and the owner recorded in assignment_inv is the last
// writer: elect the highest j.
__device__ __forceinline__ void elect_bidder(const int *bid, const float *bid_increments, const float *max_increments, int *max_idx, int j, int last)
{
    const int bid_id = bid[j];
    const float bid_inc = bid_increments[j], max_inc = max_increments[bid_id];
    if (last || in_election_window(bid_inc, max_inc)) atomicMax(&max_idx[bid_id], j);
}

// Assign for bidder j of object bid_id, elected or not, plus its part of the next round's bidder list
__device__ __forceinline__ void assign_bidder(const EmdRoundCloud &c, int j, int bid_id, bool elected, int last)
{
    if (last) {
        // every remaining bidder takes its object (not a bijection, emd_cuda.cu:201)
        c.assignment[j] = bid_id;
        atomicAdd(&c.price[bid_id], c.bid_increments[j]);
        if (elected) {
            c.assignment_inv[bid_id] = j;
            c.max_increments[bid_id] = -1e9f;
            c.max_idx[bid_id] = -1;
        }
    } else if (elected) {
        const int prev = c.assignment_inv[bid_id];
        if (prev != -1) {
            c.assignment[prev] = -1;
            const int pos = atomicAdd(c.cnt_next, 1);
            c.list_next[pos] = prev;
        }
        c.assignment_inv[bid_id] = j;
        c.assignment[j] = bid_id;
        const float np_ = __fadd_rn(c.price[bid_id], c.bid_increments[j]);
        c.price[bid_id] = np_;
        if (c.price_s) c.price_s[4 * (size_t)c.pos_of[bid_id]] = np_;
        c.max_increments[bid_id] = -1e9f;
        // elections are per round; only this thread's own comparison needed the value, every other bidder of the object
        // compares != j
        c.max_idx[bid_id] = -1;
    } else {
        const int pos = atomicAdd(c.cnt_next, 1);
        c.list_next[pos] = j;
    }
}

// GetMax and Assign of one round by ONE workgroup of BLOCK threads.  Phase 1 elects (atomicMax, performed in L2), the block
// barrier separates it from phase 2, which reads the elections with L1-bypassing loads.
template <int BLOCK>
__device__ __forceinline__ void resolve_round(const EmdRoundCloud &c, int U, int last)
{
    for (int u = threadIdx.x; u < U; u += BLOCK) elect_bidder(c.bid, c.bid_increments, c.max_increments, c.max_idx, c.list[u], last);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int u = threadIdx.x; u < U; u += BLOCK) {
        const int j = c.list[u];
        const int bid_id = c.bid[j];
        const bool elected = __hip_atomic_load(&c.max_idx[bid_id], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == j;
        assign_bidder(c, j, bid_id, elected, last);
    }
}

// ---------------- CalcDist (emd_cuda.cu:217-226) and the gradient (:284-300), per point ----------------
template <int FMA>
__device__ __forceinline__ float calc_dist_point(const float *p1, const float *p2)
{
    return sqdist<FMA>(p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]);
}

__device__ __forceinline__ void grad_point(const float *p1, const float *p2, float *o, float grad_dist)
{
    const float g = __fmul_rn(grad_dist, 2.0f);
    o[0] = __fadd_rn(o[0], __fmul_rn(g, p1[0] - p2[0]));
    o[1] = __fadd_rn(o[1], __fmul_rn(g, p1[1] - p2[1]));
    o[2] = __fadd_rn(o[2], __fmul_rn(g, p1[2] - p2[2]));
}

}  // namespace genpc
