// hpr_accept.hip -- hidden-point removal, the accept pass (hpr.hip describes the whole): the points whose own direction
// separates them are visible without a polygon; the others are listed per view, in order, and the segments of the polygon
// store are laid out from the per-view counts.
#include "hpr.h"

namespace genpc {

constexpr int kHprBatchA = 64;     // tiles per round of the accept pass

// Early accept.  If the point's own direction is already a separating normal -- u.p'_j < |p'_i| for every other
// point, i.e. the origin of the (a, b) plane satisfies every constraint strictly -- the polygon contains a disc
// around the origin and the point is visible; no polygon has to be built.  That is the case for most visible
// points (on a smooth patch nothing projects farther along the point's own ray direction).  The test is one dot
// product per candidate, tiles are skipped with the cone bound for the single normal n = u (D = 0), and the
// margin (1e-8 of the larger |p'|) is far above anything roundoff does to the clipped polygon, so the answer
// agrees with the full computation.  Points that fail go through hpr_kernel as before.
__global__ __launch_bounds__(kHprThreads) void hpr_accept_kernel(int n, const double *__restrict__ fl_all, const int *__restrict__ perm,
                                                                const HprTile *__restrict__ tiles_all, unsigned char *__restrict__ hard,
                                                                unsigned char *__restrict__ vis, int *__restrict__ cnt, int nviews)
{
    __shared__ double4 s_stage[kHprThreads];
    __shared__ unsigned long long s_mask;
    const int tid = threadIdx.x;
    const int ntiles = ceil_div_dev(n, kHprThreads);
    int view, own;
    hpr_block(ntiles, nviews, view, own);
    const double *fl = fl_all + (size_t)view * n * 3;
    const int pos = own * kHprThreads + tid;
    const HprTile *tiles = tiles_all + (size_t)view * ntiles;
    HprFrame f;
    bool active = false;
    if (pos < n) active = hpr_frame(fl + (size_t)pos * 3, f);
    const bool valid = active;
    bool ok = active;
    HprTile *s_rec = (HprTile *)s_stage;
    for (int step0 = 0; step0 < 2 * ntiles; step0 += kHprBatchA) {
        if (__syncthreads_count(active) == 0) break;
        if (tid < kHprBatchA) {
            const int tile = hpr_tile_of(step0 + tid, own);
            if (tile >= 0 && tile < ntiles) s_rec[tid] = tiles[tile];
        }
        if (tid == 0) s_mask = 0ull;
        __syncthreads();
        unsigned long long mine = 0ull;
        if (active) {
            for (int b = 0; b < kHprBatchA; b++) {
                const int tile = hpr_tile_of(step0 + b, own);
                if (tile < 0 || tile >= ntiles) continue;
                const HprTile &T = s_rec[b];
                bool need = !(T.cos_phi > 0.0);
                if (!need) {
                    // max over the tile of u.q <= rho_max cos(max(0, angle(u, w) - phi)); needed unless that is
                    // below |p'_i| minus the margin of the candidate test
                    const double uw = f.ux * T.wx + f.uy * T.wy + f.uz * T.wz;
                    const double rr = f.rho * (1.0 - 1e-7) * T.inv_rho_max;
                    if (uw >= T.cos_phi * (1.0 - 1e-9)) {
                        need = !(rr > 1.0);
                    } else {
                        const double rhs = rr - 1e-9 - T.cos_phi * uw;
                        const double s2 = T.sin2_phi * ((1.0 - uw * uw) * (1.0 + 1e-9) + 1e-12);
                        need = !(rhs > 0.0 && s2 < rhs * rhs);
                    }
                }
                if (need) mine |= 1ull << b;
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
            const int tile = hpr_tile_of(step0 + b, own);
            const int tile0 = tile * kHprThreads;
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
            if (active && ((mine >> b) & 1ull)) {
                // The test has a margin of 1e-8 |p'| and only ever ACCEPTS (a point it turns down takes the exact path), so
                // its arithmetic need not be the oracle's: fused multiply-adds, and the point itself recognised by its
                // position instead of by value (14 -> 8 instructions per candidate; the kernel is VALU-bound).
                const double lim = f.rho - 1e-8 * f.rho;          // C < thr  <=>  u.q > lim
                const int self_t = tile == own ? tid : -1;
                bool bad = false;
#pragma unroll 8
                for (int t = 0; t < kHprThreads; t++) {
                    const double4 q = s_stage[t];          // rows past the end are NaN: the comparison below is false
                    const double d = __builtin_fma(f.uz, q.z, __builtin_fma(f.uy, q.y, f.ux * q.x));
                    bad |= t != self_t && d > lim;
                }
                if (bad) { ok = false; active = false; }
            }
            __syncthreads();
        }
    }
    if (pos < n) {
        hard[(size_t)view * n + pos] = (valid && !ok) ? 1 : 0;
        vis[(size_t)view * n + perm[(size_t)view * n + pos]] = ok ? 1 : 0;          // (the polygon kernel overwrites its own points)
    }
    const int c = __syncthreads_count(ok);
    if (tid == 0 && c) atomicAdd(&cnt[view], c);
}

// The points the accept pass left over, per view in Morton order: hardlist[view][rank] = position, hardcnt[view].
// One block per view; an order-preserving scan (the order defines who shares a block of hpr_kernel).
__global__ __launch_bounds__(1024) void hpr_compact_kernel(int n, const unsigned char *__restrict__ hard, int *__restrict__ hardlist,
                                                          int *__restrict__ hardcnt)
{
    __shared__ int s_w[16];
    __shared__ int s_base;
    const int view = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int p0 = 0; p0 < n; p0 += 1024) {
        const int pos = p0 + tid;
        const bool h = pos < n && hard[(size_t)view * n + pos];
        const unsigned long long bal = __ballot(h);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_w[wave] = __popcll(bal);
        __syncthreads();
        int wbase = 0, total = 0;
        for (int w = 0; w < 16; w++) {
            wbase += w < wave ? s_w[w] : 0;
            total += s_w[w];
        }
        const int base = s_base;
        if (h) hardlist[(size_t)view * n + base + wbase + before] = pos;
        __syncthreads();
        if (tid == 0) s_base = base + total;
        __syncthreads();
    }
    if (tid == 0) hardcnt[view] = s_base;
}

// The segment record (hpr.h: HprSegs) from the views' counts
// (also clears the work counters of the wave-per-point passes: kHprWorkWords ints, a 128-byte line per counter)
__global__ __launch_bounds__(1024) void hpr_segs_kernel(int c, const int *__restrict__ hardcnt, HprSegs *__restrict__ out, int cap, int *__restrict__ work)
{
    __shared__ int s_per[8];
    if (threadIdx.x < kHprWorkWords) work[threadIdx.x] = 0;
    if (threadIdx.x < 8) s_per[threadIdx.x] = 0;
    __syncthreads();
    const int on = (c & 7) == 0 ? 1 : 0;
    int mine = 0;            // (thread t takes views t, t + 1024, ...: all of one segment)
    for (int v = threadIdx.x; v < c; v += 1024) mine += hardcnt[v];
    if (mine) atomicAdd(&s_per[on ? (threadIdx.x & 7) : 0], mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        int at = 0;            // (the sum is at most views x points < 2^31)
        for (int x = 0; x < 8; x++) { out->base[x] = at; at += s_per[x]; }
        out->base[8] = at;
        out->on = on;
        out->cap = cap;
    }
}

bool hpr_launch_accept(const HprPlan &plan, const HprCall &k, hipStream_t stream)
{
    const int n = k.n, c = k.c;
    hipLaunchKernelGGL(hpr_accept_kernel, dim3(plan.ntiles * c), dim3(kHprThreads), 0, stream, n, (const double *)k.fl, (const int *)k.i1,
                       (const HprTile *)k.tiles, k.hard, k.visible, k.counts, c);
    hipLaunchKernelGGL(hpr_compact_kernel, dim3(c), dim3(1024), 0, stream, n, (const unsigned char *)k.hard, k.hardlist, k.hardcnt);
    if (plan.prune && !check(hipMemsetAsync(k.und, 0, sizeof(int) * (size_t)c, stream), "hipMemsetAsync(hpr und)")) return false;
    hipLaunchKernelGGL(hpr_segs_kernel, dim3(1), dim3(1024), 0, stream, c, (const int *)k.hardcnt, k.segs(), (int)plan.park_cap, k.work);
    return true;
}

}  // namespace genpc
