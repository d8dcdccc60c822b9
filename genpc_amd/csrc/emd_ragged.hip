// emd_ragged.hip -- the auction (emd.hip) over a ragged batch: c independent pairs, pair j of N_j points and N_j objects
// (N_j % 256 == 0, or 0), packed in pair order, one call.  One offset table serves both clouds and every state array; it
// rides in the kernel arguments together with the bid launch's plan (emd_ragged_plan.h), so nothing is copied, nothing read
// back and nothing synchronised.  Pair j's dist, assignment, assignment_inv, bid and bid_increments are the bits of
// genpc_emd_forward(1, N_j, N_j, ...) on that pair alone; indices count inside the pair.
// A call is 2 * iters + 2 launches whatever c is (the bound include/genpc_hip.h states is 3 * iters + 2):
//   * emd_ragged_init_kernel: every pair's initial state (emd_module.alloc_state's values: assignment / assignment_inv -1,
//     the rest 0 -- the caller's outputs may be uninitialised), the round-0 bidder lists (everybody bids), the counts and
//     the filter seeds (second = -1).
//   * per round, emd_ragged_bid_kernel: emd_bid_kernel's tiled bid over ALL of the pair's objects -- (x, y, z, price) planes
//     in LDS, the fp32 squared-space pre-filter (filter_cb) seeded by the point's last best and second-best object, the
//     double-precision bid, P lanes per bidder merged with xor-shuffles, the exact-tie re-scan with the reference's
//     thread-major key computed from the pair's own N_j and bidder count U_j.  Pair j owns the fixed run of workgroups the
//     plan gave it; a workgroup finds its pair by a binary search of the table (uniform: scalar loads) and strides over the
//     pair's current U_j bidders.  The late-round object split of the dense kernel (parts / arrive tickets) is left out:
//     no workgroup waits for, or hands anything to, another.
//   * per round, emd_ragged_resolve_kernel: emd_resolve_kernel with per-pair bases -- one 1024-thread workgroup per pair,
//     GetMax, the block barrier, Assign, and the next round's bidder list.  The forced last round is as there.
//   * emd_ragged_calc_dist_kernel: CalcDist (assignment < 0 -> 0).
// Every loop is bounded by a table entry or by a count an earlier launch finished writing.  Scratch (kWsEmdRagged): two
// bidder lists and the seeds, an int per point each, and two counts per pair.
// A bidder none of whose candidates compares above -1e9 (its own coordinates are not finite) bids on object -1 in the
// reference and in genpc_emd_forward -- an out-of-bounds write; here it bids on object 0 of its pair.
#include "emd.h"
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
    constexpr int kTile = TILE, kLoadsPerThread = TILE / 256;
    __shared__ __attribute__((aligned(16))) float sX[kTile], sY[kTile], sZ[kTile], sP[kTile];
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
    const float *__restrict__ X2 = a.xyz2 + (size_t)base * 3;
    const float *__restrict__ PR = a.price + base;
    const int *__restrict__ L = (cur ? a.list_b : a.list_a) + base;
    int *__restrict__ BID = a.bid + base;
    int *__restrict__ SEC = a.second + base;

    // the reference's partition of THIS pair, needed only to order exactly tied candidates
    const int block_cnt = n / 256;
    const int unass_per_block = (U + block_cnt - 1) / block_cnt;
    const int thread_per_unass = 256 / unass_per_block;

    const int NB = (int)(((long long)U * P + kEBlock - 1) / kEBlock);
    for (int unit = bx; unit < NB; unit += G) {
        // the next tile's loads are in flight while this one is scanned (emd_bid_kernel, one tile ahead)
        float4 pre[kLoadsPerThread];
        auto fetch = [&](int k2) {
#pragma unroll
            for (int i = 0; i < kLoadsPerThread; i++) {
                const int k = k2 + threadIdx.x + i * kEBlock;
                const int kk = k < n ? k : n - 1;
                pre[i] = make_float4(X2[(size_t)kk * 3 + 0], X2[(size_t)kk * 3 + 1], X2[(size_t)kk * 3 + 2], PR[kk]);
            }
        };
        fetch(0);
        const int u = unit * per_block + wave * per_wave + g;
        const bool active = u < U;
        int j = L[active ? u : U - 1];
        j = (unsigned)j < (unsigned)n ? j : 0;              // (a list entry is a point of the pair)
        const float x1 = X1[(size_t)j * 3 + 0], y1 = X1[(size_t)j * 3 + 1], z1 = X1[(size_t)j * 3 + 2];
        float best = -1e9f, better = -1e9f;
        int best_i = -1, better_i = -1;
        // the pre-filter's seed: the point's last best and second-best object at today's prices (emd_bid_kernel)
        float seed = -1e9f;
        {
            const int sa = BID[j], sc = SEC[j];
            if (sc >= 0 && sc < n && sa != sc && (unsigned)sa < (unsigned)n) {
                const float da = bid_value<FMA>(x1, y1, z1, X2[(size_t)sa * 3 + 0], X2[(size_t)sa * 3 + 1], X2[(size_t)sa * 3 + 2], PR[sa]);
                const float dc = bid_value<FMA>(x1, y1, z1, X2[(size_t)sc * 3 + 0], X2[(size_t)sc * 3 + 1], X2[(size_t)sc * 3 + 2], PR[sc]);
                seed = fminf(da, dc);
            }
        }
        float cb = filter_cb(fmaxf(better, seed));

        for (int k2 = 0; k2 < n; k2 += kTile) {             // block-uniform trip count
            const int end_k = min(n, k2 + kTile) - k2;
            __syncthreads();                                // the previous tile has been scanned
#pragma unroll
            for (int i = 0; i < kLoadsPerThread; i++) {
                const int t = threadIdx.x + i * kEBlock;
                if (t < end_k) { sX[t] = pre[i].x; sY[t] = pre[i].y; sZ[t] = pre[i].z; sP[t] = pre[i].w; }
            }
            __syncthreads();
            if (k2 + kTile < n) fetch(k2 + kTile);
            // emd_bid_kernel's filter, operation for operation: four consecutive objects per lane and trip (4 P divides every
            // tile length: N_j % 256 == 0, P <= 64), a candidate that fails  sq < (cb - price)^2  provably evaluates to
            // d <= better, so skipping it changes no bit
            const v2f x1v = {x1, x1}, y1v = {y1, y1}, z1v = {z1, z1};
            for (int t = 4 * p; t < end_k; t += 4 * P) {
                const float4 X4 = *(const float4 *)&sX[t], Y4 = *(const float4 *)&sY[t], Z4 = *(const float4 *)&sZ[t],
                             W4 = *(const float4 *)&sP[t];
                const v2f cbv = {cb, cb};
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
                            const bool gt = d > best;
                            const bool gt2 = !gt && d > better;
                            const int kk = k2 + t + i;
                            better_i = gt ? best_i : (gt2 ? kk : better_i);
                            better = __builtin_amdgcn_fmed3f(d, best, better);
                            best = fmaxf(best, d);
                            best_i = gt ? kk : best_i;
                        }
                    }
                    cb = filter_cb(fmaxf(better, seed));
                }
            }
        }
        // merge the P partial top-2s of a bidder (value-symmetric)
        for (int off = 1; off < P; off <<= 1) {
            const float ob = __shfl_xor(best, off, kWave);
            const float obb = __shfl_xor(better, off, kWave);
            const int oi = __shfl_xor(best_i, off, kWave);
            const int obi = __shfl_xor(better_i, off, kWave);
            merge_top2(best, better, best_i, better_i, ob, obb, oi, obi);
        }
        // exact tie for first place: the candidate the reference's scan of this pair meets first
        const bool tie = active && (best == better);
        if (__any(tie)) {
            unsigned long long key = ~0ull;
            if (tie) {
                for (int k = p; k < n; k += P) {
                    const float d = bid_value<FMA>(x1, y1, z1, X2[(size_t)k * 3 + 0], X2[(size_t)k * 3 + 1], X2[(size_t)k * 3 + 2], PR[k]);
                    if (d == best) {
                        const int kt = k & 2047;                       // position in the reference's 2048-tile
                        const int tile0 = k - kt;
                        const int end_k = min(n, tile0 + 2048) - tile0;
                        const int delta = (end_k + thread_per_unass - 1) / thread_per_unass;
                        const unsigned long long kk = ((unsigned long long)(kt / delta) << 32) | (unsigned)k;
                        key = kk < key ? kk : key;
                    }
                }
            }
            for (int off = 1; off < P; off <<= 1) {
                const unsigned long long o = __shfl_xor(key, off, kWave);
                key = o < key ? o : key;
            }
            if (tie && key != ~0ull) best_i = (int)(key & 0xffffffffu);
        }
        if (active && p == 0) {
            const float inc = __fadd_rn(__fsub_rn(best, better), a.eps);
            const int o = (unsigned)best_i < (unsigned)n ? best_i : 0;      // (see the head of the file)
            BID[j] = o;
            SEC[j] = better_i;
            a.bid_increments[base + j] = inc;
            atomic_max_float(&a.max_increments[base + o], inc);
        }
    }
}

// emd_resolve_kernel (emd.hip) with per-pair bases: blockIdx.x is the pair
__global__ __launch_bounds__(kEmdRaggedResolveBlock) void emd_ragged_resolve_kernel(EmdRaggedArgs a, int cur, int last)
{
    const int pair = blockIdx.x;
    const int base = a.t.off[pair], n = a.t.off[pair + 1] - base;
    const int *__restrict__ list = (cur ? a.list_b : a.list_a) + base;
    int *__restrict__ list_next = (cur ? a.list_a : a.list_b) + base;
    int *__restrict__ cnt_next = (cur ? a.cnt_a : a.cnt_b) + pair;
    int U = (cur ? a.cnt_b : a.cnt_a)[pair];
    U = U < n ? U : n;
    int *__restrict__ assignment = a.assignment + base, *__restrict__ assignment_inv = a.assignment_inv + base;
    int *__restrict__ max_idx = a.max_idx + base;
    const int *__restrict__ bid = a.bid + base;
    float *__restrict__ price = a.price + base, *__restrict__ max_increments = a.max_increments + base;
    const float *__restrict__ bid_increments = a.bid_increments + base;
    for (int u = threadIdx.x; u < U; u += kEmdRaggedResolveBlock) {
        const int j = list[u];
        const int bid_id = bid[j];
        const double bid_inc = (double)bid_increments[j];
        const double max_inc = (double)max_increments[bid_id];
        if (last || (bid_inc - 1e-6 <= max_inc && max_inc <= bid_inc + 1e-6)) atomicMax(&max_idx[bid_id], j);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int u = threadIdx.x; u < U; u += kEmdRaggedResolveBlock) {
        const int j = list[u];
        const int bid_id = bid[j];
        const bool elected = __hip_atomic_load(&max_idx[bid_id], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == j;
        if (last) {
            // every remaining bidder takes its object (not a bijection, emd_cuda.cu:201)
            assignment[j] = bid_id;
            atomicAdd(&price[bid_id], bid_increments[j]);
            if (elected) {
                assignment_inv[bid_id] = j;
                max_increments[bid_id] = -1e9f;
                max_idx[bid_id] = -1;
            }
        } else if (elected) {
            const int prev = assignment_inv[bid_id];
            if (prev != -1) {
                assignment[prev] = -1;
                const int pos = atomicAdd(cnt_next, 1);
                list_next[pos] = prev;
            }
            assignment_inv[bid_id] = j;
            assignment[j] = bid_id;
            price[bid_id] = __fadd_rn(price[bid_id], bid_increments[j]);
            max_increments[bid_id] = -1e9f;
            max_idx[bid_id] = -1;
        } else {
            const int pos = atomicAdd(cnt_next, 1);
            list_next[pos] = j;
        }
    }
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
    const float *p1 = a.xyz1 + (size_t)t * 3;
    const float *p2 = a.xyz2 + ((size_t)base + k) * 3;
    a.dist[t] = sqdist<FMA>(p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]);
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
    const float *p1 = a.xyz1 + (size_t)t * 3;
    const float *p2 = a.xyz2 + ((size_t)base + k) * 3;
    const float g = __fmul_rn(a.grad_dist[t], 2.0f);
    float *o = a.grad_xyz + (size_t)t * 3;
    o[0] = __fadd_rn(o[0], __fmul_rn(g, p1[0] - p2[0]));
    o[1] = __fadd_rn(o[1], __fmul_rn(g, p1[1] - p2[1]));
    o[2] = __fadd_rn(o[2], __fmul_rn(g, p1[2] - p2[2]));
}

// Checks the caller's table.  1: there is work; 0: nothing to do; -1: refused, the error recorded under `who`.
static int emd_ragged_check(const char *who, int c, const int *off)
{
    RaggedTable rt;
    int max_targets = 0;
    const char *err = nullptr;
    char msg[160];
    const int rc = ragged_table_fill(c, off, off, rt, &max_targets, &err);
    if (rc < 0) {
        snprintf(msg, sizeof msg, "%s: %s", who, err);
        set_error(msg);
        return -1;
    }
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
