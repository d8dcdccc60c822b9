// emd_ragged.hip -- the auction (emd.hip) over a ragged batch: c independent pairs, pair j of N_j points and N_j objects
// (N_j % 256 == 0, or 0), packed in pair order, one call.  One offset table serves both clouds and every state array; it
// rides in the kernel arguments together with the bid launch's plan (emd_ragged_plan.h), so nothing is copied, nothing read
// back and nothing synchronised.  Pair j's dist, assignment, assignment_inv, bid and bid_increments are the bits of
// genpc_emd_forward(1, N_j, N_j, ...) on that pair alone; indices count inside the pair.
// A call is 2 * iters + 2 launches whatever c is (the bound include/genpc_hip.h states is 3 * iters + 2):
//   * emd_ragged_init_kernel: every pair's initial state (emd_module.alloc_state's values: assignment / assignment_inv -1,
//     the rest 0 -- the caller's outputs may be uninitialised), the round-0 bidder lists (everybody bids), the counts and
//     the filter seeds (second = -1).
//   * per round, emd_ragged_bid_kernel: the tiled bid it shares with emd_bid_kernel (emd_steps.h: bid_fetch, bid_tile_step,
//     bid_merge_lanes, bid_break_tie, bid_write, on a view of the pair) over ALL of the pair's objects -- (x, y, z, price) planes
//     in LDS, the fp32 squared-space pre-filter (filter_cb) seeded by the point's last best and second-best object, the
//     double-precision bid, P lanes per bidder merged with xor-shuffles, the exact-tie re-scan with the reference's
//     thread-major key computed from the pair's own N_j and bidder count U_j.  Pair j owns the fixed run of workgroups the
//     plan gave it; a workgroup finds its pair by a binary search of the table (uniform: scalar loads) and strides over the
//     pair's current U_j bidders.  The late-round object split of the dense kernel (parts / arrive tickets) is left out:
//     no workgroup waits for, or hands anything to, another.
//   * per round, emd_ragged_resolve_kernel: the body it shares with emd_resolve_kernel (resolve_round: elect_bidder, the block
//     barrier, assign_bidder and the next round's bidder list) -- one 1024-thread workgroup per pair.  The forced last round is
//     as there.
//   * emd_ragged_calc_dist_kernel: CalcDist (calc_dist_point; assignment < 0 -> 0).
// Every loop is bounded by a table entry or by a count an earlier launch finished writing.  Scratch (kWsEmdRagged): two
// bidder lists and the seeds, an int per point each, and two counts per pair.
// A bidder none of whose candidates compares above -1e9 (its own coordinates are not finite) bids on object -1 in the
// reference and in genpc_emd_forward -- an out-of-bounds write; here it bids on object 0 of its pair.
#include "emd_steps.h"
#include "emd_ragged_plan.h"
#include "ragged_table.h"
#include "../../include/genpc_hip.h"

namespace genpc {

static_assert(kEmdRaggedMaxPairs == kRaggedMaxPairs && kEmdRaggedBlock == kEBlock, "the plan header restates these");

struct EmdRaggedArgs {
    EmdRaggedTable t;
    const float *xyz1, *xyz2;
    float *dist, *price, *bid_increments, *max_increments;
    int *assignment, *assignment_inv, *bid, *max_idx;
    int *list_a, *list_b, *second;     // [off[c]] each, pair j's piece at off[j]
    int *cnt_a, *cnt_b;                // [c]
    float eps;
};
static_assert(sizeof(EmdRaggedArgs) + 64 <= 4096, "the tables must fit the kernel arguments");

constexpr int kEmdRaggedResolveBlock = 1024;

// blocks 0 .. ceil(off[c] / 256) - 1 own 256 consecutive positions of ONE pair (every N_j is a multiple of 256)
__global__ __launch_bounds__(kEBlock) void emd_ragged_init_kernel(EmdRaggedArgs a)
{
    const int total = a.t.off[a.t.c];
    const int t0 = blockIdx.x * kEBlock, t = t0 + threadIdx.x;
    if (t0 < total) {
        const int pair = emd_ragged_pair_of_point(a.t, t0);
        a.assignment[t] = -1;
        a.assignment_inv[t] = -1;
        a.price[t] = 0.0f;
        a.bid[t] = 0;
        a.bid_increments[t] = 0.0f;
        a.max_increments[t] = 0.0f;
        a.max_idx[t] = 0;
        a.dist[t] = 0.0f;
        a.list_a[t] = t - a.t.off[pair];
        a.second[t] = -1;
    }
    if (t < a.t.c) {
        a.cnt_a[t] = a.t.off[t + 1] - a.t.off[t];
        a.cnt_b[t] = 0;
    }
}

template <int FMA, int TILE>
__global__ __launch_bounds__(kEBlock) void emd_ragged_bid_kernel(EmdRaggedArgs a, int cur, int force_p)
{
    constexpr int kTile = TILE;
    __shared__ BidTile<TILE> tile;
    const int pair = emd_ragged_pair_of_block(a.t, blockIdx.x);
    const int bx = blockIdx.x - a.t.first[pair], G = a.t.first[pair + 1] - a.t.first[pair];
    const int base = a.t.off[pair], n = a.t.off[pair + 1] - base;
    const int *__restrict__ cnt = cur ? a.cnt_b : a.cnt_a;
    int *__restrict__ cnt_next = cur ? a.cnt_a : a.cnt_b;
    const int U = cnt[pair];
    if (bx == 0 && threadIdx.x == 0) cnt_next[pair] = 0;    // filled by this round's resolve
    if (U <= 0 || n <= 0 || U > n) return;                  // (U <= n by construction: a bound of every loop below)
    const int P = force_p > 0 ? force_p : pick_p(U, G);
    const int per_wave = kWave / P;
    const int per_block = kEBlock / P;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int p = lane & (P - 1);
    const int g = lane / P;

    const float *__restrict__ X1 = a.xyz1 + (size_t)base * 3;
    const int *__restrict__ L = (cur ? a.list_b : a.list_a) + base;
    EmdBidCloud c;
    c.n = n; c.U = U; c.eps = a.eps;
    c.X2 = a.xyz2 + (size_t)base * 3; c.PR = a.price + base;
    c.bid = a.bid + base; c.second = a.second + base;
    c.bid_increments = a.bid_increments + base; c.max_increments = a.max_increments + base;

    const int NB = (int)(((long long)U * P + kEBlock - 1) / kEBlock);
    for (int unit = bx; unit < NB; unit += G) {
        // the next tile's loads are in flight while this one is scanned (emd_bid_kernel, one tile ahead)
        float4 pre[TILE / 256];
        bid_fetch<TILE>(pre, c, 0);
        const int u = unit * per_block + wave * per_wave + g;
        const bool active = u < U;
        int j = L[active ? u : U - 1];
        j = (unsigned)j < (unsigned)n ? j : 0;              // (a list entry is a point of the pair)
        const float x1 = X1[(size_t)j * 3 + 0], y1 = X1[(size_t)j * 3 + 1], z1 = X1[(size_t)j * 3 + 2];
        // the pre-filter's seed: the point's last best and second-best object at today's prices (emd_bid_kernel)
        float seed = -1e9f;
        {
            const int sa = c.bid[j], sc = c.second[j];
            if (sc >= 0 && sc < n && sa != sc && (unsigned)sa < (unsigned)n) seed = seed_of_two<FMA>(x1, y1, z1, c.X2, c.PR, sa, sc);
        }
        const BidPoint pt = {x1, y1, z1, seed};
        BidLane s = bid_lane(seed);
        for (int k2 = 0; k2 < n; k2 += kTile)               // block-uniform trip count
            bid_tile_step<FMA, TILE>(tile, pre, c, pt, s, p, P, k2, k2 + kTile, n);
        bid_merge_lanes(s, P);
        bid_break_tie<FMA>(c, pt, s, active, p, P);
        if (active && p == 0) {
            int object;
            bid_write<true>(c, s, j, object);               // (object -1 becomes object 0: see the head of the file)
        }
    }
}

// emd_resolve_kernel (emd.hip) on a pair: blockIdx.x is the pair, no cell-sorted copy
__global__ __launch_bounds__(kEmdRaggedResolveBlock) void emd_ragged_resolve_kernel(EmdRaggedArgs a, int cur, int last)
{
    const int pair = blockIdx.x;
    const int base = a.t.off[pair], n = a.t.off[pair + 1] - base;
    int U = (cur ? a.cnt_b : a.cnt_a)[pair];
    U = U < n ? U : n;
    EmdRoundCloud c;
    c.list = (cur ? a.list_b : a.list_a) + base; c.list_next = (cur ? a.list_a : a.list_b) + base;
    c.cnt_next = (cur ? a.cnt_a : a.cnt_b) + pair;
    c.assignment = a.assignment + base; c.assignment_inv = a.assignment_inv + base; c.max_idx = a.max_idx + base;
    c.bid = a.bid + base; c.bid_increments = a.bid_increments + base;
    c.price = a.price + base; c.max_increments = a.max_increments + base;
    c.pos_of = nullptr; c.price_s = nullptr;
    resolve_round<kEmdRaggedResolveBlock>(c, U, last);
}

// emd_cuda.cu:217-226, a workgroup's 256 points belong to one pair
template <int FMA>
__global__ __launch_bounds__(kEBlock) void emd_ragged_calc_dist_kernel(EmdRaggedArgs a)
{
    const int total = a.t.off[a.t.c];
    const int t0 = blockIdx.x * kEBlock, t = t0 + threadIdx.x;
    if (t0 >= total) return;
    const int pair = emd_ragged_pair_of_point(a.t, t0);
    const int base = a.t.off[pair], n = a.t.off[pair + 1] - base;
    const int k = a.assignment[t];
    if (k < 0 || k >= n) {            // iters == 0: the reference would read out of bounds
        a.dist[t] = 0.0f;
        return;
    }
    a.dist[t] = calc_dist_point<FMA>(a.xyz1 + (size_t)t * 3, a.xyz2 + ((size_t)base + k) * 3);
}

struct EmdRaggedGradArgs {
    EmdRaggedTable t;
    const float *xyz1, *xyz2, *grad_dist;
    const int *idx;
    float *grad_xyz;
};

// emd_cuda.cu:284-300 (emd_grad_kernel) with per-pair bases
__global__ __launch_bounds__(kEBlock) void emd_ragged_grad_kernel(EmdRaggedGradArgs a)
{
    const int total = a.t.off[a.t.c];
    const int t0 = blockIdx.x * kEBlock, t = t0 + threadIdx.x;
    if (t0 >= total) return;
    const int pair = emd_ragged_pair_of_point(a.t, t0);
    const int base = a.t.off[pair], n = a.t.off[pair + 1] - base;
    const int k = a.idx[t];
    if (k < 0 || k >= n) return;      // (an index outside the pair: nothing to add)
    grad_point(a.xyz1 + (size_t)t * 3, a.xyz2 + ((size_t)base + k) * 3, a.grad_xyz + (size_t)t * 3, a.grad_dist[t]);
}

// Checks the caller's table.  1: there is work; 0: nothing to do; -1: refused, the error recorded under `who`.
static int emd_ragged_check(const char *who, int c, const int *off)
{
    RaggedTable rt;
    int max_targets = 0;
    const char *err = nullptr;
    char msg[160];
    const int rc = ragged_table_fill(c, off, off, rt, &max_targets, &err);
    if (rc < 0) return ragged_refuse(who, err);
    for (int j = 0; j < c; j++) {
        if ((off[j + 1] - off[j]) % 256 != 0) {
            snprintf(msg, sizeof msg, "%s: pair %d has %d points, not a multiple of 256", who, j, off[j + 1] - off[j]);
            set_error(msg);
            return -1;
        }
    }
    return rc;
}

}  // namespace genpc

GENPC_API int genpc_emd_forward_ragged(int c, const int *off, const float *xyz1, const float *xyz2, float *dist, int *assignment,
                                       float *price, int *assignment_inv, int *bid, float *bid_increments, float *max_increments,
                                       int *max_idx, float eps, int iters, void *stream)
{
    using namespace genpc;
    const int rc = emd_ragged_check("genpc_emd_forward_ragged", c, off);
    if (rc < 0) return -1;
    if (iters < 0) {
        set_error("genpc_emd_forward_ragged: negative number of rounds");
        return -1;
    }
    if (rc == 0) return 1;
    if (!xyz1 || !xyz2 || !dist || !assignment || !price || !assignment_inv || !bid || !bid_increments || !max_increments || !max_idx) {
        set_error("genpc_emd_forward_ragged: null pointer");
        return -1;
    }
    hipStream_t st = (hipStream_t)stream;
    const int total = off[c];
    const bool fma = arith_mode() != 0;
    EmdRaggedArgs a{};
    const int grid = emd_ragged_plan(c, off, num_cus(), a.t);
    a.xyz1 = xyz1; a.xyz2 = xyz2; a.dist = dist; a.price = price; a.bid_increments = bid_increments; a.max_increments = max_increments;
    a.assignment = assignment; a.assignment_inv = assignment_inv; a.bid = bid; a.max_idx = max_idx; a.eps = eps;
    WsLayout L;
    L.add(a.list_a, (size_t)total);
    L.add(a.list_b, (size_t)total);
    L.add(a.second, (size_t)total);
    L.add(a.cnt_a, (size_t)c);
    L.add(a.cnt_b, (size_t)c);
    if (!ws_alloc(L, kWsEmdRagged, st)) return 0;

    const int lin_blocks = ceil_div(total, kEBlock);
    // the init launch also writes the c counts, one thread each: at least ceil(c / 256) blocks (384 pairs, one of them with points)
    const int init_blocks = lin_blocks > ceil_div(c, kEBlock) ? lin_blocks : ceil_div(c, kEBlock);
    hipLaunchKernelGGL(emd_ragged_init_kernel, dim3(init_blocks), dim3(kEBlock), 0, st, a);
    // 1024-object tiles where the bid is throughput-bound, 2048 for a small call (emd.hip measured both); every choice gives the same bits
    const bool small_tile = total > 8192;
    typedef void (*bid_fn)(EmdRaggedArgs, int, int);
    const bid_fn f = small_tile ? (fma ? emd_ragged_bid_kernel<1, 1024> : emd_ragged_bid_kernel<0, 1024>)
                                : (fma ? emd_ragged_bid_kernel<1, 2048> : emd_ragged_bid_kernel<0, 2048>);
    for (int it = 0; it < iters; it++) {
        const int cur = it & 1;
        // lanes per bidder as emd.hip picks them: from round 1 on the seeds make the filter selective, and one bidder per wave
        // keeps one bidder's exact evaluations from stalling another's lanes -- unless many pairs are in flight
        const int force_p = it > 0 && c < 32 ? 64 : 0;
        hipLaunchKernelGGL(f, dim3(grid), dim3(kEBlock), 0, st, a, cur, force_p);
        hipLaunchKernelGGL(emd_ragged_resolve_kernel, dim3(c), dim3(kEmdRaggedResolveBlock), 0, st, a, cur, it == iters - 1 ? 1 : 0);
    }
    if (fma) hipLaunchKernelGGL((emd_ragged_calc_dist_kernel<1>), dim3(lin_blocks), dim3(kEBlock), 0, st, a);
    else hipLaunchKernelGGL((emd_ragged_calc_dist_kernel<0>), dim3(lin_blocks), dim3(kEBlock), 0, st, a);
    return check(hipGetLastError(), "emd ragged forward launch") ? 1 : 0;
}

GENPC_API int genpc_emd_backward_ragged(int c, const int *off, const float *xyz1, const float *xyz2, float *gradxyz,
                                        const float *graddist, const int *idx, void *stream)
{
    using namespace genpc;
    const int rc = emd_ragged_check("genpc_emd_backward_ragged", c, off);
    if (rc < 0) return -1;
    if (rc == 0) return 1;
    if (!xyz1 || !xyz2 || !gradxyz || !graddist || !idx) {
        set_error("genpc_emd_backward_ragged: null pointer");
        return -1;
    }
    EmdRaggedGradArgs a{};
    emd_ragged_plan(c, off, 1, a.t);
    a.xyz1 = xyz1; a.xyz2 = xyz2; a.grad_dist = graddist; a.idx = idx; a.grad_xyz = gradxyz;
    hipLaunchKernelGGL(emd_ragged_grad_kernel, dim3(ceil_div(off[c], kEBlock)), dim3(kEBlock), 0, (hipStream_t)stream, a);
    return check(hipGetLastError(), "emd_ragged_grad_kernel launch") ? 1 : 0;
}
