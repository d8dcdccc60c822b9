// emd_grid.hip -- the auction's Bid step (emd_cuda.cu:95-179) with the objects a bidder tests CULLED.
//
// The reference's Bid evaluates every (unassigned point, object) pair of a round; so did emd_bid_kernel (emd.hip) --
// behind a squared-distance pre-filter, but every bidder still walked all n objects (64 MB of L2 -> LDS per late
// round at n = 16384).  Objects never move; only prices rise, and prices are >= 0 (they start at
// 0 and every increment is best - better + eps >= eps >= 0).  An object can change a bidder's (best, better) only if
// its value 3 - |x2 - x1| - price exceeds m = max(better so far, seed), hence only if its squared distance is below
// fl(cb^2), cb = filter_cb(m) -- the pre-filter's own threshold at price 0 (emd.h).  So the objects are sorted ONCE
// per call into a uniform grid (grid.h: cell_grid_build_kernel, counting sort in LDS, cells numbered
// x-fastest so that the cells [cx0, cx1] of a (cy, cz) ROW are one contiguous run of the sorted array), and a bidder
// visits only the rows of the box |p - x1| <= cb around itself whose (y, z) gap is below cb -- with the bound of
// grid.h, every rounding accounted for: a skipped row provably holds nothing that could matter, what is visited
// goes through the SAME per-object pre-filter and the SAME exact fp64 value as before, every object at most once.
// The top-2 VALUES (duplicates count) and the index of a unique best are therefore the reference's; an exact tie for
// first place takes the thread-major re-scan of the tiled kernel unchanged.  Bit-identical assignments and prices
// (tests/test_gpu_emd.py: every parity test runs both bid kernels).
//
// Seeds: from its second bid on a point is seeded with the values, at today's prices, of the two objects it ranked
// first and second last time (as in the tiled kernel); a point that has not bid yet first probes the 3 x 3 rows
// around its own cell (x range +-1 cell), takes the second-best value found as its seed and skips those cells in the
// main pass.  Simulated on uniform clouds a late-round bidder then meets ~30 of 16384 objects, on a partial scan
// against its ground truth 50-350 (tools: /tmp experiment recorded in DESIGN.md section 4.3).
// Prices live twice: price[] in the caller's object order (the ABI's array) and the .w of the sorted entries, which
// the settle / resolve kernels keep in step (pos_of[object]) -- a bidder reads (x, y, z, price) as ONE 16-byte entry,
// consecutive lanes consecutive entries; the object's index (orig_of) is read only for the rare entry that passes.
#include "emd.h"
#include "../../include/genpc_hip.h"

#include <stdlib.h>

namespace genpc {

// pmin[batch][c] = the smallest price among the objects of cell c as the sorted copy holds them now, +inf for an empty cell.
// Prices only rise: a table computed before any later round stays a lower bound.
__global__ __launch_bounds__(256) void emd_cell_pmin_kernel(int cells_max, const CellGridHdr *__restrict__ hdr, const int *__restrict__ start,
                                                            const float4 *__restrict__ sorted, int n, float *__restrict__ pmin)
{
    const int batch = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (c > cells_max) return;
    float m = __builtin_inff();
    if (c < hdr[batch].cells) {
        const int *st = start + (size_t)batch * (cells_max + 1);
        const float4 *S = sorted + (size_t)batch * n;
        const int e = st[c + 1];
        for (int p = st[c]; p < e; p++) m = fminf(m, S[p].w);
    }
    pmin[(size_t)batch * (cells_max + 1) + c] = m;
}

// The Bid step of one round over the grid.  Same outputs as emd_bid_kernel (emd.hip): bid, second, bid_increments,
// max_increments, the chain records.  LPB lanes share a bidder (a power of two, 8 .. 64, picked per round from the
// number of bidders like pick_p); a lane takes whole rows of the bidder's box.
template <int FMA>
__global__ __launch_bounds__(kEBlock) __attribute__((amdgpu_waves_per_eu(4, 8))) void emd_bid_grid_kernel(EmdGridBid a)
{
    __shared__ int s_pre[kEBlock / kWave][72], s_p0[kEBlock / kWave][72];      // per wave: (64 / LPB) groups x (LPB + 1) entries
    __shared__ int s_que[kEBlock / kWave][512];                                 // per wave: (64 / LPB) groups x 8 LPB queued entries
    const int n = a.n, G = a.G, nb = a.nb;
    // Clouds interleaved over the block ids (and with them over the XCDs): the clouds of a call differ in work here --
    // bidders left, sizes of their boxes; a mis-framed scan keeps ten times the work of its neighbours -- and
    // emd_bid_kernel's "a cloud's blocks on one XCD" (its objects stay in that XCD's L2) made the launch as long as
    // the heaviest cloud on an eighth of the chip.
    const int batch = blockIdx.x % nb, bx = blockIdx.x / nb;
    const int U = a.cnt[batch];
    if (bx == 0 && threadIdx.x == 0) a.cnt_next[batch] = 0;   // filled by this round's settle / resolve
    if (a.feedback != nullptr && blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(a.feedback, U, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (U == 0) return;
    int LPB = a.force_lpb > 0 ? a.force_lpb : pick_p(U, G);
    if (a.force_lpb <= 0 && a.lpb_max > 0 && LPB > a.lpb_max) LPB = a.lpb_max;
    LPB = LPB < 8 ? 8 : LPB;
    const int per_wave = kWave / LPB, per_block = kEBlock / LPB;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int sub = lane & (LPB - 1), grp = lane / LPB;
    const size_t base = (size_t)batch * n;
    const float *__restrict__ X1 = a.xyz1 + base * 3;
    const float *__restrict__ X2 = a.xyz2 + base * 3;
    const float *__restrict__ PR = a.price + base;
    const int *__restrict__ L = a.list + base;
    const float4 *__restrict__ S = a.sorted + base;      // (x, y, z, price) in cell order: settle / resolve keep .w in step
    const int *__restrict__ OF = a.orig_of + base;       // object index of a sorted position: read only for the rare object that passes
    const int *__restrict__ ST = a.start + (size_t)batch * (a.cells_max + 1);
    const float *__restrict__ PM = a.cell_pmin ? a.cell_pmin + (size_t)batch * (a.cells_max + 1) : nullptr;
    const CellGridHdr H = a.hdr[batch];
    const int gx = H.g[0], gy = H.g[1], gz = H.g[2];
    const float h = H.h, inf = __builtin_inff();
    // reference partition, needed only to order exactly tied candidates
    const int thread_per_unass = ref_thread_per_unass(n, U);

    const int units = (U + per_block - 1) / per_block;
    for (int unit = bx; unit < units; unit += G) {
        const int u = unit * per_block + wave * per_wave + grp;
        const bool active = u < U;
        const int j = L[active ? u : U - 1];
        const float x1 = X1[(size_t)j * 3 + 0], y1 = X1[(size_t)j * 3 + 1], z1 = X1[(size_t)j * 3 + 2];
        float best = -1e9f, better = -1e9f;
        int best_i = -1, better_i = -1;
        float seed = -1e9f;
        bool seeded = false;
        unsigned st_rows = 0, st_kept = 0, st_items = 0, st_pass = 0;      // hook counters (a.stats != null only)
        int mode = 0;                           // what a batch does with an entry: 0 bid, 1 collect the objects tied for first place, 2 proxy scan
        unsigned long long tie_key = ~0ull;
        float k1 = inf, k2 = inf;               // proxy scan: the two smallest sqrtf(sq) + price of this lane and where
        int q1 = -1, q2 = -1;
        {
            const int sa = a.bid[base + j], sc = a.second[base + j];
            if (sc >= 0 && sa != sc && (unsigned)sa < (unsigned)n) {
                seed = seed_of_two<FMA>(x1, y1, z1, X2, PR, sa, sc);
                seeded = true;
            }
        }
        float cb = filter_cb(fmaxf(better, seed));
        const float sx = grid_slack(H.slack[0], x1), sy = grid_slack(H.slack[1], y1), sz = grid_slack(H.slack[2], z1);
        // One batch of runs of the sorted array, one per lane ([pA, pA + lA), possibly empty), spread
        // EVENLY over the group's lanes: exclusive scan of the lengths, then lane `sub` takes the items sub, sub + LPB, ...
        // of the concatenation (a run of a dense row is hundreds of objects: a lane per row left 63 lanes waiting for one --
        // the 13 bundled scans took 196 ms against 62 for the tiled kernel).  Consecutive lanes read consecutive entries.
        // Per item: the pre-filter, the exact value, the lane-local top-2 -- four loads in flight.
        int *pre = s_pre[wave] + grp * (LPB + 1), *pp0 = s_p0[wave] + grp * (LPB + 1);
        int *que = s_que[wave] + grp * (8 * LPB);
        int qn = 0;                              // queued entries (the same number in every lane of the group)
        const unsigned long long gmask = LPB == 64 ? ~0ull : (((1ull << LPB) - 1ull) << (lane & ~(LPB - 1)));
        // the queued entries, one per lane: exact value (emd_cuda.cu:142-146), lane-local top-2 (or the tie key), then a
        // tighter threshold for what follows: the largest lane-local second-best of the group is the value of a second object
        auto flush = [&]() {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int e = sub; e < qn; e += LPB) {
                const int ps = que[e];
                const float4 o = S[ps];
                st_pass++;
                const float d = bid_value<FMA>(x1, y1, z1, o.x, o.y, o.z, o.w);
                if (mode == 0) {
                    insert_top2(best, better, best_i, better_i, d, OF[ps]);
                } else if (d == best) {
                    // an object that ties for first place: its key in the reference's thread-major scan order
                    // (emd_cuda.cu:108-118,136-139,165-173: the candidate the scan meets first is reported)
                    const unsigned long long kk = ref_tie_key(OF[ps], n, thread_per_unass);
                    tie_key = kk < tie_key ? kk : tie_key;
                }
            }
            qn = 0;
            if (mode == 0) {
                float gb = better;
                for (int off = 1; off < LPB; off <<= 1) gb = fmaxf(gb, __shfl_xor(gb, off, kWave));
                seed = fmaxf(seed, gb);
                cb = filter_cb(fmaxf(better, seed));
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        };
        auto batch_eval = [&](int pA, int lA) {
            // The non-empty runs of this batch (one per lane at most) are compacted into the group's LDS list -- start and
            // length -- and then walked RUN BY RUN: the group's lanes stride a run together (consecutive lanes, consecutive
            // 16-byte entries), four runs' first strides in flight at a time.  (Round 4 concatenated the runs and dealt the
            // concatenation evenly over the lanes: every entry then cost a cursor walk over the run boundaries -- dependent LDS
            // reads -- on top of an exclusive scan per batch: ~100 lane-operations per object tested on the 13 bundled scans,
            // where a bidder's ball holds ~680 objects in ~84 short rows; VERDICT r4 weak #3.)
            const unsigned long long mA = __ballot(lA > 0) & gmask;
            const int E = __popcll(mA);
            if (lA > 0) { const int e = __popcll(mA & ((1ull << lane) - 1ull)); pre[e] = lA; pp0[e] = pA; }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            auto test = [&](const float4 &o, int pos, bool in) -> bool {
                if (!in) return false;
                const float sq = sqdist<FMA>(o.x - x1, o.y - y1, o.z - z1);
                if (mode == 2) {
                    const float key = sqrtf(sq) + o.w;
                    if (key < k1) { k2 = k1; q2 = q1; k1 = key; q1 = pos; }
                    else if (key < k2) { k2 = key; q2 = pos; }
                    return false;
                }
                const float tt = cb - o.w;
                return sq < tt * tt;
            };
            auto enqueue = [&](bool pass, int pos) {
                // entries that pass the filter are QUEUED, not valued on the spot: the exact path (sqrt, fp64) is ~50
                // instructions that the whole wave executes whenever any lane passes
                const unsigned long long m = __ballot(pass) & gmask;
                if (pass) que[qn + __popcll(m & ((1ull << lane) - 1ull))] = pos;
                qn += __popcll(m);
            };
            int longest = 0;
            for (int e0 = 0; e0 < E; e0 += 4) {            // group-uniform trip counts throughout
                float4 o[4];
                int ps[4];
                bool in[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const bool have = e0 + i < E;
                    const int p0 = have ? pp0[e0 + i] : pp0[0], ln = have ? pre[e0 + i] : 0;
                    longest = max(longest, ln);
                    in[i] = sub < ln;
                    ps[i] = p0 + (in[i] ? sub : 0);
                    o[i] = S[ps[i]];
                    if (sub == 0) st_items += (unsigned)ln;
                }
                bool pass[4];
#pragma unroll
                for (int i = 0; i < 4; i++) pass[i] = test(o[i], ps[i], in[i]);
                if (mode != 2 && (__ballot(pass[0] | pass[1] | pass[2] | pass[3]) & gmask) != 0ull) {
#pragma unroll
                    for (int i = 0; i < 4; i++) enqueue(pass[i], ps[i]);
                    if (qn > 4 * LPB) flush();
                }
            }
            // what the runs hold beyond one stride of the group (dense rows: hundreds of entries), two strides in flight
            if (longest > LPB) {
                for (int e = 0; e < E; e++) {
                    const int ln = pre[e];
                    if (ln <= LPB) continue;
                    const int p0 = pp0[e];
                    for (int off0 = LPB; off0 < ln; off0 += 2 * LPB) {
                        const int a0 = off0 + sub, a1 = off0 + LPB + sub;
                        const bool i0 = a0 < ln, i1 = a1 < ln;
                        const float4 oa = S[p0 + (i0 ? a0 : 0)], ob = S[p0 + (i1 ? a1 : 0)];
                        const bool pa_ = test(oa, p0 + a0, i0), pb_ = test(ob, p0 + a1, i1);
                        if (mode != 2 && (__ballot(pa_ | pb_) & gmask) != 0ull) {
                            enqueue(pa_, p0 + a0);
                            enqueue(pb_, p0 + a1);
                            if (qn > 4 * LPB) flush();
                        }
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();       // the lists are rewritten by the next batch
        };
        const int cqx = grid_cell1(x1, H.lo[0], H.inv, gx), cqy = grid_cell1(y1, H.lo[1], H.inv, gy), cqz = grid_cell1(z1, H.lo[2], H.inv, gz);
        const bool cull = !H.bad && (fabsf(x1) + fabsf(y1)) + fabsf(z1) < inf;
        // the box |p - x1| <= cb (cell function monotone: a point within cb of x1 on an axis lies in [cell(x1 - cb), cell(x1 + cb)])
        int bx0 = 0, bx1 = gx - 1, by0 = 0, by1 = gy - 1, bz0 = 0, bz1 = gz - 1;
        auto set_box = [&](float R) {
            { const GridRange r = grid_cell_range(x1, R, sx, H.lo[0], H.inv, gx); bx0 = r.c0; bx1 = r.c1; }
            { const GridRange r = grid_cell_range(y1, R, sy, H.lo[1], H.inv, gy); by0 = r.c0; by1 = r.c1; }
            { const GridRange r = grid_cell_range(z1, R, sz, H.lo[2], H.inv, gz); bz0 = r.c0; bz1 = r.c1; }
        };
        if (cull) set_box(cb);
        // A point without a seed (its first bid) or with a stale one (the prices of the two objects it knew have risen since
        // it last bid: on a partial scan against its ground truth the boxes grew to 200 rows and 4000 objects per bidder):
        // the 3 x 3 x 3 cells around it are scanned with a cheap fp32 proxy of the value (sqrtf(sq) + price, smaller is
        // better); the two best-looking objects are then VALUED exactly, like the seeds of a point that has bid before
        // -- the second-best over all objects is at least the smaller of any two -- and the box shrinks to what can still
        // beat that.  (Letting the lanes run the exact path on whatever they meet first cost 41 fp64 evaluations per point
        // in round 0, where every lane's first two objects pass the filter: 115 us for 16384 points; and with 8 points
        // to a wave on the 13 scans the exact path, taken whenever ANY lane passes, was half of the kernel's instructions.)
        if (cull && (!seeded || (by1 - by0 + 1) * (bz1 - bz0 + 1) > kTwoPassRows)) {
            mode = 2;
            const int ex0 = max(0, cqx - 1), ex1 = min(gx - 1, cqx + 1);
            for (int r0 = 0; r0 < 9; r0 += LPB) {
                const int r = r0 + sub;
                const int cy = cqy + r % 3 - 1, cz = cqz + r / 3 - 1;
                int pA = 0, lA = 0;
                if (r < 9 && cy >= 0 && cy < gy && cz >= 0 && cz < gz) {
                    const int row = (cz * gy + cy) * gx;
                    pA = ST[row + ex0];
                    lA = ST[row + ex1 + 1] - pA;
                }
                batch_eval(pA, lA);
            }
            mode = 0;
            for (int off = 1; off < LPB; off <<= 1) {
                const float o1 = __shfl_xor(k1, off, kWave), o2 = __shfl_xor(k2, off, kWave);
                const int p1 = __shfl_xor(q1, off, kWave), p2 = __shfl_xor(q2, off, kWave);
                // two smallest of {k1, k2, o1, o2} (the lanes' sets are disjoint)
                if (o1 < k1) { k2 = fminf(k1, o2) == k1 ? k1 : o2; q2 = (k1 <= o2) ? q1 : p2; k1 = o1; q1 = p1; }
                else { const bool t = o1 < k2; k2 = t ? o1 : k2; q2 = t ? p1 : q2; }
            }
            if (q2 >= 0) {
                const float4 oa = S[q1], ob = S[q2];
                seed = fmaxf(seed, fminf(bid_value<FMA>(x1, y1, z1, oa.x, oa.y, oa.z, oa.w), bid_value<FMA>(x1, y1, z1, ob.x, ob.y, ob.z, ob.w)));
                cb = filter_cb(seed);
                set_box(cb);
            }
        }
        auto sweep = [&]() {
        const int wy = by1 - by0 + 1, nrows = wy * (bz1 - bz0 + 1);
        for (int r0 = 0; r0 < nrows; r0 += LPB) {         // group-uniform trip count
            const int r = r0 + sub;
            int pA = 0, lA = 0;
            // cells of the row that can still hold a candidate at today's prices (bit i: cell cx0 + i) and the non-empty ones
            // that cannot; first cell of the row's range
            unsigned long long km = 0ull, cm = 0ull;
            int cbase = 0;
            if (r < nrows) {
                st_rows++;
                const int rz = r / wy;
                const int cy = by0 + (r - rz * wy), cz = bz0 + rz;
                int cx0 = bx0, cx1 = bx1;
                bool keep = true;
                float lb0 = 0.0f;
                if (cull) {
                    // the row's (y, z) gap against the threshold; what is left of it bounds |dx|: the box becomes a ball
                    const float gyv = grid_gap(cy, 1, gy, H.lo[1], h, y1, sy), gzv = grid_gap(cz, 1, gz, H.lo[2], h, z1, sz);
                    lb0 = __fmaf_rn(gyv, gyv, __fmul_rn(gzv, gzv));
                    const float lb = lb0 * kGridShrink;
                    const float c2 = __fmul_rn(cb, cb);
                    keep = lb < c2;                          // else nothing in this row can matter (prices >= 0)
                    if (keep) {
                        const float W = sqrtf(fmaxf(0.0f, __fmul_rn(c2, 1.000001f) - lb)) * 1.000001f;
                        const GridRange rw = grid_cell_range_in(x1, W, sx, H.lo[0], H.inv, gx, bx0, bx1);
                        cx0 = rw.c0;
                        cx1 = rw.c1;
                    }
                }
                if (keep && cx0 <= cx1) {
                    st_kept++;
                    const int row = (cz * gy + cy) * gx;
                    const int wdt = cx1 - cx0 + 1;
                    if (PM != nullptr && cull && wdt <= 64) {
                        // Cell by cell with the prices in: an object of cell c is at least the cell's gap away and costs at
                        // least the cell's smallest price p, so it can pass the filter (sq < (cb - price)^2, cb - price > 0)
                        // only if gap^2 < (cb - p)^2 -- on a partial scan against its ground truth the ball of a late-round
                        // bidder holds ~680 objects, all but two of them priced out.
                        cbase = row + cx0;
                        for (int i0 = 0; i0 < wdt; i0 += 4) {
                            float pm[4];
#pragma unroll
                            for (int k = 0; k < 4; k++) pm[k] = i0 + k < wdt ? PM[cbase + i0 + k] : inf;
#pragma unroll
                            for (int k = 0; k < 4; k++) {
                                if (!(pm[k] < inf)) continue;              // empty (or past the range)
                                const float gxv = grid_gap(cx0 + i0 + k, 1, gx, H.lo[0], h, x1, sx);
                                const float lbc = __fmaf_rn(gxv, gxv, lb0) * kGridShrink;
                                const float tt = cb - pm[k];
                                const bool kc = tt > 0.0f && lbc < tt * tt;
                                km |= kc ? 1ull << (i0 + k) : 0ull;
                                cm |= kc ? 0ull : 1ull << (i0 + k);
                            }
                        }
                    } else {
                        pA = ST[row + cx0];
                        lA = ST[row + cx1 + 1] - pA;
                    }
                }
            }
            if (PM == nullptr) {
                batch_eval(pA, lA);
            } else {
                // a row's kept cells as runs of the sorted array: one run from a kept cell to the last kept cell in front of
                // the next priced-out one (empty cells in between cost nothing); most rows give one run, some two
                do {
                    if (km) {
                        const int s = __ffsll((long long)km) - 1;
                        const unsigned long long above = cm & ~((2ull << s) - 1ull);
                        const unsigned long long seg = above ? km & ((1ull << (__ffsll((long long)above) - 1)) - 1ull) : km;
                        const int e = 63 - __clzll((long long)seg);
                        pA = ST[cbase + s];
                        lA = ST[cbase + e + 1] - pA;
                        km &= ~seg;
                    }
                    batch_eval(pA, lA);
                    pA = 0; lA = 0;
                } while ((__ballot(km != 0ull) & gmask) != 0ull);
            }
        }
        };
        sweep();
        flush();
        // merge the LPB partial top-2s of a bidder (value-symmetric)
        for (int off = 1; off < LPB; off <<= 1) {
            const float ob = __shfl_xor(best, off, kWave), obb = __shfl_xor(better, off, kWave);
            const int oi = __shfl_xor(best_i, off, kWave), obi = __shfl_xor(better_i, off, kWave);
            merge_top2(best, better, best_i, better_i, ob, obb, oi, obi);
        }
        // exact tie for first place: pick the candidate the reference's scan meets first (emd_bid_kernel's path)
        const bool tie = active && (best == better);
        if (a.stats) {
            unsigned v[4] = {st_rows, st_kept, st_items, st_pass};
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (!active) v[q] = 0;
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) v[q] += __shfl_xor(v[q], o);
            }
            const unsigned long long nb_act = __popcll(__ballot(active && sub == 0)), nb_tie = __popcll(__ballot(tie && sub == 0)),
                                     nb_uns = __popcll(__ballot(active && sub == 0 && !seeded));
            if (lane == 0) {
                atomicAdd(&a.stats[0], nb_act);
                atomicAdd(&a.stats[1], (unsigned long long)v[0]);
                atomicAdd(&a.stats[2], (unsigned long long)v[1]);
                atomicAdd(&a.stats[3], (unsigned long long)v[2]);
                atomicAdd(&a.stats[4], (unsigned long long)v[3]);
                atomicAdd(&a.stats[5], nb_tie);
                atomicAdd(&a.stats[6], nb_uns);
            }
        }
        // Exact tie for first place: the reference reports the tied object its thread-major scan meets first.  The tied
        // objects have the value `best`, so they lie inside the ball of anything worth more than the next float below it:
        // ONE more culled sweep finds them all (the tiled kernel re-scans all n objects with the fp64 value -- a single tie
        // held a whole launch for ~200 us at n = 16384, and a partial scan against its ground truth has a tie in most rounds).
        if (__any(tie)) {
            if (tie) {
                mode = 1;
                cb = filter_cb(__uint_as_float(__float_as_uint(best) + (best > 0.0f ? -1 : (best < 0.0f ? 1 : 0))));      // the float below `best` (a +-0 best: itself; 3 - r - p = 0 only for objects ~3 away)
                if (best == 0.0f) cb = filter_cb(-1e-30f);
                bx0 = 0; bx1 = gx - 1; by0 = 0; by1 = gy - 1; bz0 = 0; bz1 = gz - 1;
                if (cull) set_box(cb);
                sweep();            // (a group's batches use only its own lanes: the other groups of the wave sit this out)
                flush();
            }
            for (int off = 1; off < LPB; off <<= 1) {
                const unsigned long long o = __shfl_xor(tie_key, off, kWave);
                tie_key = o < tie_key ? o : tie_key;
            }
            if (tie) best_i = (int)(tie_key & 0xffffffffu);
        }
        if (active && sub == 0) {
            const float inc = __fadd_rn(__fsub_rn(best, better), a.eps);
            a.bid[base + j] = best_i;
            a.second[base + j] = better_i;
            a.bid_increments[base + j] = inc;
            atomic_max_float(&a.max_increments[base + best_i], inc);
            if (a.chain_head != nullptr) {
                const unsigned long long mine = ((unsigned long long)(unsigned)__float_as_int(inc) << 32) | (a.stamp << 24) | (unsigned)j;
                a.chain_next[base + j] = atomicExch(&a.chain_head[base + best_i], mine);
                atomicAdd(&a.chain_cnt[base + best_i], 1);
            }
        }
    }
}

int launch_emd_cell_pmin(int b, int cells_max, const CellGridHdr *hdr, const int *start, const float4 *sorted, int n, float *pmin, hipStream_t st)
{
    hipLaunchKernelGGL(emd_cell_pmin_kernel, dim3(ceil_div(cells_max + 1, 256), b), dim3(256), 0, st, cells_max, hdr, start, sorted, n, pmin);
    return check(hipGetLastError(), "emd_cell_pmin_kernel launch") ? 1 : 0;
}

int launch_emd_bid_grid(const EmdGridBid &a, int fma, hipStream_t st)
{
    if (fma) hipLaunchKernelGGL((emd_bid_grid_kernel<1>), dim3(a.G * a.nb), dim3(kEBlock), 0, st, a);
    else hipLaunchKernelGGL((emd_bid_grid_kernel<0>), dim3(a.G * a.nb), dim3(kEBlock), 0, st, a);
    return 1;
}

}  // namespace genpc
