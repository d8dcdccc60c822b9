// hpr_first.hip -- hidden-point removal, the first polygon pass (hpr.hip describes the whole): one thread per point the accept
// pass left over, its polygon in LDS; and the pruning of views for genpc_hpr_best_view_counts.
#include "hpr.h"

namespace genpc {

HPR_PROF_ARRAY(hpr_first_prof_read)

constexpr int kHprBatch = 64;      // tiles tested per round (one bit each)
constexpr int kHprRimStep = 8;     // after this many tiles ...
constexpr double kHprRimD2 = 1.0e6; // ... a polygon with a vertex farther than 1000 from the origin is a silhouette point's
                                   // ... and is handed to the second pass if the cloud has at least kHprRimTiles tiles

// status[kHprStListed] = points handed to the wave-per-point pass, status[kHprStError] = error (2: a polygon outgrew kHprOverCap),
// status[kHprStParked] = points left undecided by the split first kernel (continued by the wave-per-point pass)
__global__ __launch_bounds__(kHprThreads) void hpr_kernel(int n, const double *__restrict__ fl_all, const int *__restrict__ perm,
                                                         const HprTile *__restrict__ tiles_all, const int *__restrict__ hardlist,
                                                         const int *__restrict__ hardcnt, unsigned char *__restrict__ vis,
                                                         int *__restrict__ cnt, int *status, int *__restrict__ over_list, int no_cull, int max_clips,
                                                         int split, int4 *__restrict__ surv, double2 *__restrict__ surv_poly,
                                                         int *__restrict__ und, int straggle_from, int straggle_lanes, int nviews, int home_tiles, const HprSegs *__restrict__ segs_p, int chunk_w, int home_chunks)
{
    HPR_PROF_DECL;
    const HprSegs segs = *segs_p;
    __shared__ double2 s_poly[kHprMaxV * kHprThreads];
    __shared__ double4 s_stage[kHprThreads];      // 64 tile records while testing, then one tile's candidates
    __shared__ unsigned long long s_mask;
    static_assert(sizeof(HprTile) * kHprBatch <= sizeof(double4) * kHprThreads, "the tile records share the staging area");
    const int tid = threadIdx.x;
    int view, blk;
    hpr_block(ceil_div_dev(n, kHprThreads), nviews, view, blk);
    const double *fl = fl_all + (size_t)view * n * 3;
    // block g of a view owns the points of rank 128 g .. 128 g + 127 in the view's list of points the accept pass
    // left over; its tile order starts at the tile of its middle point (hpr_base_tile: the oracle's rule too)
    const int nhard = hardcnt[view];
    if (blk * kHprThreads >= nhard) return;
    const int *hl = hardlist + (size_t)view * n;
    const int rank = blk * kHprThreads + tid;
    const int pos = rank < nhard ? hl[rank] : -1;
    const int i = pos >= 0 ? perm[(size_t)view * n + pos] : -1;
    const int ntiles = ceil_div_dev(n, kHprThreads), own = hpr_base_tile(hl, nhard, rank);
    const HprTile *tiles = tiles_all + (size_t)view * ntiles;
    HprFrame f;
    bool active = false;
    int nv = 0;            // > 0 visible so far, 0 hidden, -1 handed to the second pass
    if (i >= 0) active = hpr_frame(fl + (size_t)pos * 3, f);
    double2 *poly = s_poly + tid;
    HprReach R = {};
    if (active) {
        nv = 4;
        poly[0 * kHprThreads] = make_double2(-kHprBox, -kHprBox);
        poly[1 * kHprThreads] = make_double2(kHprBox, -kHprBox);
        poly[2 * kHprThreads] = make_double2(kHprBox, kHprBox);
        poly[3 * kHprThreads] = make_double2(-kHprBox, kHprBox);
        R = hpr_reach(poly, kHprThreads, nv);
    }
    int nclips = 0;
    HprTile *s_rec = (HprTile *)s_stage;
    const int home = pos >= 0 ? pos / kHprThreads : -0x40000000;      // the tile this point lies in
    // Stage one tile of candidates and let the lanes that want it clip against it.  Pass 1 over the tile, the
    // same for every lane: which candidates are not provably out of reach (one bit each).  Pass 2: every lane
    // takes ITS marked candidates in order -- the lanes of a wave run their k-th marked candidate together, so
    // the wave pays for the longest list, not for the sum of all of them (clipping candidate by candidate as
    // they come costs 10x more: the lanes meet their cuts at different candidates).
    // Clip the polygon of this lane by the 128 candidates of one tile; `load(k)` returns candidate k of the tile
    // (rows past the end of the cloud: NaN).
    // Split form: a point this kernel does not finish is parked with its polygon as the exact path left it and the place
    // to resume from -- code = 256 x (home tiles done: 0 .. 3) + candidates of the next home tile already taken -- and a
    // wave of hpr_overflow_kernel continues from there (round 3 restarted such points from the box: 6.5 of 45 ms).
    auto park = [&](int code) {
        const int sx = hpr_seg_of(segs, view);
        const int slot = segs.base[sx] + atomicAdd(&status[kHprStSegFill + sx], 1);
        if (und) atomicAdd(&und[view], 1);
        if (slot >= segs.cap) {          // the polygon store is full: listed instead
            over_list[atomicAdd(&status[kHprStListed], 1)] = view * n + rank;
            nv = -1;
            active = false;
            return;
        }
        atomicAdd(&status[kHprStParked], 1);
        surv[slot] = make_int4(view * n + rank, nv, pos, code);
        double2 *sp = surv_poly + (size_t)slot * kHprMaxV;
        for (int k = 0; k < nv; k++) sp[k] = poly[k * kHprThreads];
        nv = -1;
        active = false;
    };
    auto clip_by_tile = [&](int tile, int rel, auto load) {
                // 32 candidates at a time: the marks are taken against the polygon as the previous 32 left it (while
                // the polygon is still the box every candidate is marked; after the nearest few it is tight and
                // almost none are)
                // (in the point's HOME tile the chunks start with its own: nearest neighbours first)
                const int rot = tile == home ? ((pos - home * kHprThreads) >> 5) : 0;
                for (int cc = 0; cc < (rel == 0 ? home_chunks : kHprThreads / 32) && active; cc++) {
                    const int c0 = ((cc + rot) & (kHprThreads / 32 - 1)) * 32;
                    for (int s0 = 0; s0 < 32 && active; s0 += chunk_w) {
                    // Marks: the candidates that CUT the polygon as it is now (a vertex strictly outside) -- the polygon in
                    // registers, every lane the same straight-line test.  The clip loop below runs as long as its slowest
                    // lane, at ~500 instructions a trip; with marks from the reach bounds (hpr_far: 17 of 32 candidates
                    // marked per lane, a few of them real cuts) a wave made 28 trips per 32 candidates with a third of its
                    // lanes busy (tools/hpr_phases.py).  A candidate that does not cut now cannot cut what is left later.
                    double2 pv[kHprMaxV];
#pragma unroll
                    for (int k = 0; k < kHprMaxV; k++) pv[k] = poly[(k < nv ? k : 0) * kHprThreads];
                    unsigned m = 0u;
#pragma unroll 1
                    for (int t = s0; t < s0 + chunk_w; t++) {
                        const double4 q = load(c0 + t);      // rows past the end are NaN
                        const double A = f.e1x * q.x + f.e1y * q.y + f.e1z * q.z;
                        const double B = f.e2x * q.x + f.e2y * q.y + f.e2z * q.z;
                        const double C = f.rho - (f.ux * q.x + f.uy * q.y + f.uz * q.z);
                        const bool self = q.x == f.px && q.y == f.py && q.z == f.pz;      // the point itself, or an exact duplicate
                        bool cut = false;
#pragma unroll
                        for (int k = 0; k < kHprMaxV; k++) cut |= pv[k].x * A + pv[k].y * B - C > 0.0;      // (NaN rows: false)
                        m |= (!self && cut) ? (1u << t) : 0u;
                    }
                    HPR_PROF_ADD(4, 1);                                   // marking rounds (summed over lanes)
                    HPR_PROF_ADD(7, __popc(m));                           // marked candidates (summed over lanes)
                    while (m && active) {
                        HPR_PROF_ADD(5, 1);                               // clip-loop trips (the wave's = its lanes' maximum)
                        HPR_PROF_ADD(6, 1);                               // ... summed over lanes
                        const int t = __ffs((int)m) - 1;
                        m &= m - 1;
                        const double4 q = load(c0 + t);      // (recomputed: the same values)
                        const double A = f.e1x * q.x + f.e1y * q.y + f.e1z * q.z;
                        const double B = f.e2x * q.x + f.e2y * q.y + f.e2z * q.z;
                        const double C = f.rho - (f.ux * q.x + f.uy * q.y + f.uz * q.z);
                        // outside vertices: how many, and where their (cyclic) run starts
                        // (eight vertices are fetched at a time: one LDS round trip instead of eight in a row;
                        // slots past nv are read -- they belong to this thread -- and ignored)
                        int out = 0, first = 0, runs = 0;
                        bool prev_out;
                        {
                            const double2 v = poly[(nv - 1) * kHprThreads];
                            prev_out = v.x * A + v.y * B - C > 0.0;
                        }
                        for (int k0 = 0; k0 < nv; k0 += 8) {
                            double2 v[8];
#pragma unroll
                            for (int j = 0; j < 8; j++) v[j] = poly[(k0 + j < kHprMaxV ? k0 + j : kHprMaxV - 1) * kHprThreads];
#pragma unroll
                            for (int j = 0; j < 8; j++) {
                                const bool o = k0 + j < nv && v[j].x * A + v[j].y * B - C > 0.0;
                                out += o ? 1 : 0;
                                first = (o && !prev_out) ? k0 + j : first;
                                runs += (o && !prev_out) ? 1 : 0;
                                prev_out = k0 + j < nv ? o : prev_out;
                            }
                        }
                        if (!out) continue;
                        if (out == nv) { nv = 0; active = false; break; }
                        // (runs > 1: on a sliver, roundoff can put the outside vertices in two runs; the in-place clip
                        // assumes one -- the second pass clips like the oracle does, vertex by vertex)
                        if (nv - out + 2 > kHprMaxV || runs > 1) {
                            if (split && rel >= 0) { park(rel * 256 + cc * 32 + t); break; }      // (candidate t not taken yet)
                            over_list[atomicAdd(&status[kHprStListed], 1)] = view * n + rank;
                            if (und) atomicAdd(&und[view], 1);
                            nv = -1;
                            active = false;
                            break;
                        }
                        const int mm = hpr_clip_inplace(poly, kHprThreads, nv, out, first, A, B, C);
                        if (mm < 3) { nv = 0; active = false; break; }      // no interior left: not strictly extreme
                        nv = mm;
                        // a polygon that has been cut this often is a sliver far from the origin that thousands
                        // of candidates shave a little more (seen: 1400 cuts): such a point holds its whole block
                        // up -- the second pass, a wave per point with the candidates tested in parallel, is the
                        // place for it
                        if (++nclips > max_clips) {
                            if (split && rel >= 0) { park(rel * 256 + cc * 32 + t + 1); break; }
                            over_list[atomicAdd(&status[kHprStListed], 1)] = view * n + rank;
                            if (und) atomicAdd(&und[view], 1);
                            nv = -1;
                            active = false;
                            break;
                        }
                    }
                    }
                }
                };
    // Stage one tile of candidates in LDS and let the lanes that want it clip against it.
    auto take_tile = [&](int tile, bool wanted) {
        const int tile0 = tile * kHprThreads;
        const int tn = min(kHprThreads, n - tile0);
        {
            // rows past the end are NaN: they cut nothing
            double4 q = make_double4(__builtin_nan(""), 0.0, 0.0, 0.0);
            if (tid < tn) {
                const double *g = fl + (size_t)(tile0 + tid) * 3;
                q = make_double4(g[0], g[1], g[2], 0.0);
            }
            s_stage[tid] = q;
        }
        __syncthreads();
        if (active && wanted) clip_by_tile(tile, -1, [&](int k) { return s_stage[k]; });
        __syncthreads();
    };
    // Phase 1: every point's home tile and its two neighbours, whatever the group's starting tile is (when few
    // points are left over, the 128 of a block lie many tiles apart; a polygon that has not met its nearest
    // neighbours first stays large for a long time).
    // Each lane reads ITS tiles straight from memory (its neighbours in the wave read the same or the next tile:
    // the lines are shared in L1/L2): staging them through LDS would take the block's tiles one after the other
    // with a few lanes busy on each -- measured 1.0 of a block's 2.7 ms.
    [[maybe_unused]] const unsigned long long prof_t0 = HPR_PROF_CLOCK();
    for (int rel = 0; rel < home_tiles && active; rel++) {            // home, home + 1, home - 1: nearest first
        const int tile = home + (rel == 0 ? 0 : (rel == 1 ? 1 : -1));
        if (tile < 0 || tile >= ntiles) continue;
        const int tile0 = tile * kHprThreads;
        clip_by_tile(tile, rel, [&](int k) {
            const int j = tile0 + k;
            if (j >= n) return make_double4(__builtin_nan(""), 0.0, 0.0, 0.0);
            const double *g = fl + (size_t)j * 3;
            return make_double4(g[0], g[1], g[2], 0.0);
        });
    }
    // Verify phase.  The polygon now reflects the nearest neighbours; later candidates mostly shave its corners.
    // Take its centroid (a*, b*) -- an interior point -- and test that ONE normal n = u + a* e1 + b* e2 against
    // every other point: if a* A + b* B - C < 0 with room to spare for all of them, (a*, b*) is strictly feasible,
    // the final polygon is not empty and the point is visible -- one dot product per candidate instead of the
    // polygon machinery, and tiles skipped with the same cone bound (for a one-vertex polygon).  A lane that
    // meets a counter-example goes on to phase 2 with its polygon untouched (the decision there is the same
    // computation as without this phase).  This is the early accept of hpr_accept_kernel with a better normal.
    // (Interior point: the centroid; for a polygon that runs out to the box, a point near its bounded end.)
    [[maybe_unused]] const unsigned long long prof_t1 = HPR_PROF_CLOCK();
    HPR_PROF_ADD(0, prof_t1 - prof_t0);            // home tiles
    HPR_PROF_ADD(8, 1);                            // waves
    if (!split || (no_cull & kHprBlockVerify)) {
        bool trying = active && nv >= 3;
        double2 ctr = make_double2(0.0, 0.0);
        if (trying) {
            // the two vertices nearest the origin (v0, v1) and the centroid
            double2 v0 = make_double2(0.0, 0.0), v1 = v0;
            double r0 = __builtin_inf(), r1 = __builtin_inf();
            for (int k = 0; k < nv; k++) {
                const double2 v = poly[k * kHprThreads];
                const double r2 = v.x * v.x + v.y * v.y;
                ctr.x += v.x;
                ctr.y += v.y;
                if (r2 < r0) { r1 = r0; v1 = v0; r0 = r2; v0 = v; }
                else if (r2 < r1) { r1 = r2; v1 = v; }
            }
            ctr.x /= (double)nv;
            ctr.y /= (double)nv;
            if (!(ctr.x * ctr.x + ctr.y * ctr.y < 1.0e6)) {
                // The polygon runs out to the box (a point on the silhouette): its centroid is somewhere near
                // the box.  Any point of the segment from a vertex to the centroid is interior: step from the
                // vertex nearest the origin towards the centroid by the length of the polygon's near part.
                const double dx = ctr.x - v0.x, dy = ctr.y - v0.y;
                const double len = sqrt(dx * dx + dy * dy);
                double h = sqrt((v1.x - v0.x) * (v1.x - v0.x) + (v1.y - v0.y) * (v1.y - v0.y));
                h = h < 0.5 * len ? h : 0.5 * len;
                trying = len > 0.0 && h > 0.0;
                if (trying) {
                    ctr.x = v0.x + h * (dx / len);
                    ctr.y = v0.y + h * (dy / len);
                }
            }
        }
        const double nx = f.ux + ctr.x * f.e1x + ctr.y * f.e2x, ny = f.uy + ctr.x * f.e1y + ctr.y * f.e2y,
                     nz = f.uz + ctr.x * f.e1z + ctr.y * f.e2z;
        const double nn = 1.0 + ctr.x * ctr.x + ctr.y * ctr.y;
        const double thr = 1e-10 * f.rho * nn;
        // a one-vertex "polygon" in LDS slot kHprMaxV - 1?  No: hpr_tile_needed reads through a pointer -- give it
        // a private copy (stride 0 is fine: one element)
        const double cl = sqrt(nn) * (1.0 + 1e-15), cpsi1 = 1.0 / cl, spsi1 = sqrt(nn - 1.0) / cl * (1.0 + 1e-15);
        for (int step0 = 0; step0 < 2 * ntiles; step0 += kHprBatch) {
            if (__syncthreads_count(trying) == 0) break;
            if (tid < kHprBatch) {
                const int tile = hpr_tile_of(step0 + tid, own);
                if (tile >= 0 && tile < ntiles) s_rec[tid] = tiles[tile];
            }
            if (tid == 0) s_mask = 0ull;
            __syncthreads();
            unsigned long long mine = 0ull;
            if (trying) {
                for (int b = 0; b < kHprBatch; b++) {
                    const int tile = hpr_tile_of(step0 + b, own);
                    if (tile < 0 || tile >= ntiles) continue;
                    if (hpr_tile_needed(f, cpsi1, spsi1, &ctr, 0, 1, s_rec[b])) mine |= 1ull << b;
                }
            }
            {
                unsigned long long w = mine;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) w |= (unsigned long long)__shfl_xor((long long)w, o, kWave);
                if ((tid & (kWave - 1)) == 0 && w) atomicOr(&s_mask, w);
            }
            __syncthreads();
            unsigned long long todo = s_mask;
            while (todo) {
                const int b = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int tile0 = hpr_tile_of(step0 + b, own) * kHprThreads;
                const int tn = min(kHprThreads, n - tile0);
                {
                    double4 q = make_double4(__builtin_nan(""), 0.0, 0.0, 0.0);
                    if (tid < tn) {
                        const double *g = fl + (size_t)(tile0 + tid) * 3;
                        q = make_double4(g[0], g[1], g[2], 0.0);
                    }
                    s_stage[tid] = q;
                }
                __syncthreads();
                if (trying && ((mine >> b) & 1ull)) {
                    bool bad = false;
#pragma unroll 8
                    for (int t = 0; t < kHprThreads; t++) {
                        const double4 q = s_stage[t];          // NaN rows: the comparison is false
                        const double sv = (nx * q.x + ny * q.y + nz * q.z) - f.rho;
                        const bool self = q.x == f.px && q.y == f.py && q.z == f.pz;
                        bad |= !self && sv > -thr;
                    }
                    if (bad) trying = false;
                }
                __syncthreads();
            }
        }
        if (trying) {              // no counter-example anywhere: visible
            active = false;        // (nv >= 3 stays: reported as visible below)
        }
    }
    // Split form: every other tile (outward from the group's starting tile) is the wave-per-point pass's: only about
    // one listed point in eight is still undecided here, and a block that carried them on waited for its slowest
    // lane with the other seven eighths idle (1.5 of a block's 2.7 ms).  The undecided lanes park
    // their polygons in memory; hpr_overflow_kernel continues from them, one wave each.
    [[maybe_unused]] const unsigned long long prof_t2 = HPR_PROF_CLOCK();
    HPR_PROF_ADD(1, prof_t2 - prof_t1);            // verify
    if (split && active) {
        const unsigned long long bal = __ballot(true);
        const int lane = tid & (kWave - 1);
        int base = 0;
        if (lane == __ffsll((long long)bal) - 1) {
            const int sx = hpr_seg_of(segs, view);
            base = segs.base[sx] + atomicAdd(&status[kHprStSegFill + sx], __popcll(bal));
            atomicAdd(&status[kHprStParked], min(__popcll(bal), max(segs.cap - base, 0)));
            if (und) atomicAdd(&und[view], __popcll(bal));      // (a wave's lanes share the view: one block = one view)
        }
        base = __shfl(base, __ffsll((long long)bal) - 1, kWave);
        const int slot = base + __popcll(bal & ((1ull << lane) - 1ull));
        if (slot >= segs.cap) {          // the polygon store is full: listed instead
            over_list[atomicAdd(&status[kHprStListed], 1)] = view * n + rank;
        } else {
            surv[slot] = make_int4(view * n + rank, nv, pos, home_chunks < kHprThreads / 32 ? home_chunks * 32 : home_tiles * 256);
            double2 *sp = surv_poly + (size_t)slot * kHprMaxV;
            for (int k = 0; k < nv; k++) sp[k] = poly[k * kHprThreads];
        }
        nv = -1;               // decided later
        active = false;
    }
    // split == 0 (large clouds: few views, thousands of tiles -- there the lanes of a block want the same tiles and
    // staging them once per block through LDS beats per-lane reads: 2 x 165546 points 40 ms against 49):
    // Phase 2: all other tiles, outward from the group's starting tile, in batches of 1, 1, 2, 4, ... 64 whose
    // records are tested first (the polygon is tight by now, most tiles are out of its reach)
    for (int step0 = 0, bsz = 1; step0 < 2 * ntiles; step0 += bsz, bsz = step0 < kHprBatch ? step0 : kHprBatch) {
        // A polygon that still runs out to the box after the eight nearest tiles belongs to a point on the
        // silhouette: it is cut by points all along the rim and holds its whole wave up for as many tiles as
        // the cloud has -- in a large cloud such points go to the second pass, which puts a wave on each
        // (measured: 2 x 165546 points 77 -> 51 ms; 64 x 10000 points 29 -> 32 ms, hence the size rule).
        if (step0 == kHprRimStep && ntiles >= kHprRimTiles && active && R.d2 > kHprRimD2) {
            over_list[atomicAdd(&status[kHprStListed], 1)] = view * n + rank;
                            if (und) atomicAdd(&und[view], 1);
            nv = -1;
            active = false;
        }
        const int nactive = __syncthreads_count(active);
        if (nactive == 0) break;
        // After the first few batches of tiles the points a block still carries restart in the wave-per-point pass, one
        // wave each: a block that walks on for some of its 128 points holds two waves (and their LDS) for every tile any
        // of them needs -- block times at 2 x 165546: median 3.1 M ticks, slowest 23 M = the launch -- while the
        // wave-per-point pass tests 64 candidates against one polygon at a time and clips with all lanes.  Measured
        // (hand-off from batch 4, all remaining points): 2 x 165546 21.8 -> 14.8 ms (radius 100: 30.6 -> 16.2), 64 x 10000
        // 12.1 -> 7.3 (15.7 -> 7.3); from batch 16: 9.4, from 64: 12.6.  (The split form for many views of a small cloud
        // keeps its own second kernel: 1024 x 10000 65 / 39.6 / 43.9 ms against 74 / 36.9 / 42.7 this way.)
        if (step0 >= straggle_from && nactive <= straggle_lanes) {
            if (active) {
                over_list[atomicAdd(&status[kHprStListed], 1)] = view * n + rank;
                if (und) atomicAdd(&und[view], 1);
                nv = -1;
                active = false;
            }
            break;
        }
        // which of the next tiles can still cut somebody's polygon (tested against the polygon as it is now:
        // it only shrinks, so a tile found out of reach stays out of reach)
        if (tid < bsz) {
            const int tile = hpr_tile_of(step0 + tid, own);
            if (tile >= 0 && tile < ntiles) s_rec[tid] = tiles[tile];
        }
        if (tid == 0) s_mask = 0ull;
        __syncthreads();
        unsigned long long mine = 0ull;
        if (active) {
            R = hpr_reach(poly, kHprThreads, nv);
            const double l = sqrt(1.0 + R.d2) * (1.0 + 1e-15), cpsi = 1.0 / l, spsi = sqrt(R.d2) / l * (1.0 + 1e-15);
            for (int b = 0; b < bsz; b++) {
                const int tile = hpr_tile_of(step0 + b, own);
                if (tile < 0 || tile >= ntiles) continue;
                if (tile >= home - 1 && tile <= home + 1) continue;          // taken in phase 1
                if (hpr_tile_needed(f, cpsi, spsi, poly, kHprThreads, nv, s_rec[b])) mine |= 1ull << b;
            }
        }
        {
            unsigned long long w = mine;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) w |= (unsigned long long)__shfl_xor((long long)w, o, kWave);
            if ((tid & (kWave - 1)) == 0 && w) atomicOr(&s_mask, w);
        }
        __syncthreads();
        unsigned long long todo = s_mask;
        while (todo) {
            const int b = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            take_tile(hpr_tile_of(step0 + b, own), ((mine >> b) & 1ull) != 0ull);
        }
    }
    HPR_PROF_ADD(2, HPR_PROF_CLOCK() - prof_t2);    // park / walk
    HPR_PROF_FLUSH();
    const bool seen = i >= 0 && nv > 0;
    if (i >= 0 && nv >= 0) vis[(size_t)view * n + i] = seen ? 1 : 0;
    const int c = __syncthreads_count(seen);
    if (tid == 0 && c) atomicAdd(&cnt[view], c);
}

// viewpoint_select only needs the view that sees the MOST points.  After hpr_kernel a view's count is a lower bound
// (accepted + verified + decided in phase 1) and `und` says how many of its points are still undecided: a view whose
// upper bound stays below the best lower bound cannot win (nor tie), and the second kernel and the wave-per-point
// pass skip its points.  alive[v] = 1: the view's final count is exact.
__global__ __launch_bounds__(1024) void hpr_prune_kernel(int c, const int *__restrict__ cnt, const int *__restrict__ und,
                                                        unsigned char *__restrict__ alive)
{
    __shared__ int s_max[16];
    int m = 0;
    for (int v = threadIdx.x; v < c; v += 1024) m = max(m, cnt[v]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, kWave));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = m;
    __syncthreads();
    m = s_max[0];
    for (int w = 1; w < 16; w++) m = max(m, s_max[w]);
    for (int v = threadIdx.x; v < c; v += 1024) alive[v] = cnt[v] + und[v] >= m ? 1 : 0;
}

bool hpr_launch_first(const HprPlan &plan, const HprCall &k, hipStream_t stream)
{
    hipLaunchKernelGGL(hpr_kernel, dim3(plan.ntiles * k.c), dim3(kHprThreads), 0, stream, k.n, (const double *)k.fl, (const int *)k.i1,
                       (const HprTile *)k.tiles, (const int *)k.hardlist, (const int *)k.hardcnt, k.visible, k.counts, k.status, k.list, k.no_cull,
                       plan.max_clips, plan.split, k.surv, k.surv_poly, k.und, plan.straggle_from, plan.straggle_lanes, k.c, plan.home_tiles,
                       (const HprSegs *)k.segs(), plan.chunk_w, plan.home_chunks);
    if (!check(hipGetLastError(), "hpr launch")) return false;
    if (plan.prune) hipLaunchKernelGGL(hpr_prune_kernel, dim3(1), dim3(1024), 0, stream, k.c, (const int *)k.counts, (const int *)k.und, k.alive);
    return true;
}

}  // namespace genpc
