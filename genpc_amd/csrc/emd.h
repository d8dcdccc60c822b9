// emd.h -- device helpers shared by the auction kernels (emd.hip: tiled bid, settle / resolve; emd_ragged.hip: the same over
// a ragged batch; emd_grid.hip: the cell-sorted culled bid; emd_auction.hip: all rounds in one launch): the bit-exact rules
// of the bid, its ties and the election, each stated once.  emd_steps.h builds a round's steps on ONE cloud from them for
// emd.hip and emd_ragged.hip.  The objects' spatial index is grid.h's.
#pragma once
#include "common.h"
#include "grid.h"

#include <type_traits>

namespace genpc {

typedef float v2f __attribute__((ext_vector_type(2)));
constexpr int kEBlock = 256;
// objects per LDS tile: template parameter TILE of the bid kernel, 2048 (32 KiB as float4) or 1024 (16 KiB)
constexpr int kZMax = 4;            // object slices per bidder group in the late-round split (measured best of 1..16)
constexpr int kSplitMaxBidders = 4096;   // bidders per batch element the split scratch can hold
constexpr int kArrivePerBatch = 1024;    // arrival counters per batch element (>= kSplitMaxBidders * 64 / 256)

// emd_cuda.cu:142-146
template <int FMA>
__device__ __forceinline__ float bid_value(float x1, float y1, float z1, float x2, float y2, float z2, float price)
{
    float s = sqdist<FMA>(x2 - x1, y2 - y1, z2 - z1);
    float r = sqrtf(s);   // correctly rounded (hipcc default); __fsqrt_rn is the ~1 ulp native sqrt
    return (float)((3.0 - (double)r) - (double)price);
}

// float atomic max; increments are >= 0 in every sane call (eps >= 0), where the
// int ordering of the bit patterns equals the float ordering even against the
// -1e9 reset value.  Negative values take the CAS loop of emd_cuda.cu:10-20.
__device__ __forceinline__ void atomic_max_float(float *addr, float val)
{
    if (val >= 0.0f) {
        atomicMax((int *)addr, __float_as_int(val));
    } else {
        int ret = __float_as_int(*addr);
        while (val > __int_as_float(ret)) {
            int old = ret;
            if ((ret = atomicCAS((int *)addr, old, __float_as_int(val))) == old) break;
        }
    }
}

// Folds (ob, obb, oi, obi) into (b, bb, bi, bbi): best / second-best values with the
// index of an object attaining each.  Value-symmetric; on a tie for first place the
// lower index is kept as `bi` (the reference's order is restored by the tie path).
// I: int, an object index, or long long, position << 32 | object index (emd_auction.hip: ties keep the lower POSITION -- any
// choice does: an exact tie for first place is settled by the tie path, the second's identity only seeds the next search).
template <class I>
__device__ __forceinline__ void merge_top2(float &b, float &bb, I &bi, I &bbi, float ob, float obb, I oi, I obi)
{
    typedef std::make_unsigned_t<I> UI;
    float nb2;
    I nbi;
    if (b > ob) {
        nb2 = fmaxf(bb, ob);
        nbi = ob > bb ? oi : bbi;
    } else if (ob > b) {
        nb2 = fmaxf(obb, b);
        nbi = b > obb ? bi : obi;
    } else {                       // equal first places: the other one is the second
        nb2 = b;
        nbi = ((UI)oi < (UI)bi) ? bi : oi;
    }
    const bool take = ob > b || (ob == b && (UI)oi < (UI)bi);
    bi = take ? oi : bi;
    b = fmaxf(b, ob);
    bb = nb2;
    bbi = nbi;
}

// One candidate of value d and index kk into a lane's own top-2 (v_max + v_med3): strictly greater wins, so of equal values
// the one met first is kept (I as for merge_top2).
template <class I>
__device__ __forceinline__ void insert_top2(float &best, float &better, I &best_i, I &better_i, float d, I kk)
{
    const bool gt = d > best;
    const bool gt2 = !gt && d > better;
    better_i = gt ? best_i : (gt2 ? kk : better_i);
    better = __builtin_amdgcn_fmed3f(d, best, better);
    best = fmaxf(best, d);
    best_i = gt ? kk : best_i;
}

// The reference's partition of a cloud of n objects with U bidders left (emd_cuda.cu:108-118): threads of a block that share
// one bidder.  Needed only to order exactly tied candidates.
__device__ __forceinline__ int ref_thread_per_unass(int n, int U)
{
    const int block_cnt = n / 256;
    const int unass_per_block = (U + block_cnt - 1) / block_cnt;
    return 256 / unass_per_block;
}

// Key of object k among the objects tied for a bidder's first place: (reference thread, index), thread-major as the
// reference's scan meets them (emd_cuda.cu:136-139,165-173) -- the smallest key is the object it reports.
__device__ __forceinline__ unsigned long long ref_tie_key(int k, int n, int thread_per_unass)
{
    const int kt = k & 2047;                       // position in the reference's 2048-tile
    const int tile0 = k - kt;
    const int end_k = min(n, tile0 + 2048) - tile0;
    const int delta = (end_k + thread_per_unass - 1) / thread_per_unass;
    return ((unsigned long long)(kt / delta) << 32) | (unsigned)k;
}

// GetMax's window (emd_cuda.cu:188): a bidder stands for election when its increment is within 1e-6 of the object's largest
__device__ __forceinline__ bool in_election_window(float bid_increment, float max_increment)
{
    const double bid_inc = (double)bid_increment, max_inc = (double)max_increment;
    return bid_inc - 1e-6 <= max_inc && max_inc <= bid_inc + 1e-6;
}

// Threshold of the bid pre-filter for m = max(better, seed): a candidate with squared distance sq
// and price p >= 0 can only matter if fl32((3 - sqrtf(sq)) - p) > m.  With tt = fl(cb - p), the
// test  sq < fl(tt * tt)  must pass whenever that holds.  Roundings: cb and tt (relative u each, on
// magnitudes <= 3 + |m|), the square (u), the correctly rounded sqrtf (u), the fp32 rounding of the
// value itself (2u |m|); with 0 <= p < 3 + |m| (otherwise tt <= 0 and nothing can matter) the test
// is safe iff the slack added to (3 - m) is at least u (21 + 9 |m|).  2e-6 (1 + |m|) = 33.5 u (1 + |m|).
// (The first version used the constant 2e-6: proven only for clouds in the unit cube, |m| <= 3.)
__device__ __forceinline__ float filter_cb(float m)
{
    return __fadd_rn(__fsub_rn(3.0f, m), __fmul_rn(2e-6f, __fadd_rn(1.0f, fabsf(m))));
}

// Seed of the pre-filter from two distinct objects sa, sc of the cloud (X2, PR: its objects and prices), re-valued at
// today's prices: the second-best value over ALL objects is at least the smaller of any two distinct objects' values, so
// a candidate provably not above the seed can be neither best nor strictly second.
template <int FMA>
__device__ __forceinline__ float seed_of_two(float x1, float y1, float z1, const float *__restrict__ X2, const float *__restrict__ PR, int sa, int sc)
{
    const float da = bid_value<FMA>(x1, y1, z1, X2[(size_t)sa * 3 + 0], X2[(size_t)sa * 3 + 1], X2[(size_t)sa * 3 + 2], PR[sa]);
    const float dc = bid_value<FMA>(x1, y1, z1, X2[(size_t)sc * 3 + 0], X2[(size_t)sc * 3 + 1], X2[(size_t)sc * 3 + 2], PR[sc]);
    return fminf(da, dc);
}

// lanes-per-bidder for U bidders on a grid of G blocks per batch element
__device__ __forceinline__ int pick_p(int U, int G)
{
    int P = 64;
    while (P > 1 && ((long long)U * P + kEBlock - 1) / kEBlock > G) P >>= 1;
    return P;
}

// ---- cell-sorted culled bid (emd_grid.hip) ----
constexpr int kTwoPassRows = 25;        // boxes of more (y, z) rows than this take the near cells first (both culled bid searches)
struct EmdGridBid {
    int n, G, nb, cells_max, force_lpb, lpb_max;      // lpb_max > 0: at most this many lanes per bidder
    float eps;
    unsigned stamp;
    const float *xyz1, *xyz2, *price;
    const int *list, *cnt, *start, *orig_of;
    int *cnt_next, *bid, *second;
    float *bid_increments, *max_increments;
    const float4 *sorted;
    const CellGridHdr *hdr;
    unsigned long long *chain_head, *chain_next;
    int *chain_cnt;                // bidders per object this round (emd_settle_kernel)
    int *feedback;                 // round 3 only (else null): pinned host word that receives cloud 0's bidder count (emd_auction.hip: which path suits the data)
    const float *cell_pmin;        // per cloud, cells_max + 1 floats: a lower bound of the prices in every cell, +inf for an empty one (emd_cell_pmin_kernel); null: rows are not culled by price
    unsigned long long *stats;     // hook (genpc_emd_tune): [0] bidders, [1] rows of their boxes, [2] rows kept, [3] objects tested, [4] exact evaluations, [5] first-place ties, [6] unseeded bidders; else null
};
// ---- all rounds in one launch, threads own the points (emd_auction.hip) ----
int launch_emd_auction(int b, int n, const float *xyz1, const float *xyz2, float *dist, int *assignment, float *price, int *assignment_inv,
                       int *bid, float *bid_increments, float *max_increments, int *max_idx, float eps, int iters, int fma, hipStream_t st, bool forced);
int *emd_feedback_slot(int b, int n, bool device);
// admission of launches whose workgroups wait for each other (emd_auction.hip; the multi-workgroup sampling of fps.hip takes its
// share from the same budget): quarter-CU units
bool persist_reserve(int wgs, int capacity, hipStream_t st);
void persist_commit(int wgs, hipStream_t st);
int emd_auction_capacity();
int launch_emd_bid_grid(const EmdGridBid &a, int fma, hipStream_t st);
int launch_emd_cell_pmin(int b, int cells_max, const CellGridHdr *hdr, const int *start, const float4 *sorted, int n, float *pmin, hipStream_t st);

}  // namespace genpc
