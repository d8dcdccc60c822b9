// hpr_wave.hip -- hidden-point removal, the wave-per-point passes (hpr.hip describes the whole): the decision rounds, the
// parked points' first try in a kernel of its own, the exact walk in three tiers of polygon size, and the final word on errors.
#include "hpr.h"

#include <limits.h>

namespace genpc {

HPR_PROF_ARRAY(hpr_wave_prof_read)

constexpr int kHprDecideChunk = 4;      // consecutive parked points a wave of hpr_decide_kernel takes per draw

// status[kHprStError] != 0 (an internal error) reaches the caller without a host read of it: every count becomes -1
__global__ __launch_bounds__(256) void hpr_finish_kernel(int c, const int *__restrict__ status, int *__restrict__ cnt)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v < c && status[kHprStError] != 0) cnt[v] = -1;
}

// second pass: one WAVE per listed point, polygon in LDS (two buffers of kHprOverCap vertices).  Lane b tests
// tile b of a batch of 64; in a tile that can reach the polygon the 64 lanes test 64 candidates at once, and
// the few that are not provably out of reach are taken one by one, in order, the vertex test spread over the
// lanes and the clip itself done by lane 0.  Same candidates, same order, same arithmetic as the first pass
// (and the oracle).
// hpr_clip and hpr_reach by all 64 lanes of a wave (the wave-per-point pass: its heaviest points clip 1000-2000 times
// polygons of a hundred vertices; with one lane clipping and every lane walking the whole polygon for the reach, a
// clip cost 36 k ticks and one point set the launch's 24 ms at 2 x 165546).  Every output vertex is computed by the
// expressions of hpr_clip from the same operands, the maxima of hpr_reach are exact: the polygons are the same bits.
__device__ __forceinline__ int hpr_clip_wave(const double2 *src, int nv, double A, double B, double C, double2 *dst, int lane)
{
    int base = 0;
    for (int k0 = 0; k0 < nv; k0 += kWave) {
        const int k = k0 + lane;
        bool in0 = false, cross = false;
        double2 cur = make_double2(0.0, 0.0), x = cur;
        if (k < nv) {
            const int k2 = k + 1 < nv ? k + 1 : 0;
            cur = src[k];
            const double2 nxt = src[k2];
            const double s0 = cur.x * A + cur.y * B - C;
            const double s1 = nxt.x * A + nxt.y * B - C;
            in0 = !(s0 > 0.0);
            cross = (s0 > 0.0) != (s1 > 0.0) && s0 != 0.0 && s1 != 0.0;
            if (cross) {
                const double t = s0 / (s0 - s1);
                x.x = cur.x + t * (nxt.x - cur.x);
                x.y = cur.y + t * (nxt.y - cur.y);
            }
        }
        const unsigned long long bi = __ballot(in0), bc = __ballot(cross);
        const unsigned long long lt = (1ull << lane) - 1ull;
        int pos = base + __popcll(bi & lt) + __popcll(bc & lt);
        if (in0) dst[pos++] = cur;
        if (cross) dst[pos] = x;
        base += __popcll(bi) + __popcll(bc);
    }
    return base;
}

__device__ __forceinline__ HprReach hpr_reach_wave(const double2 *p, int nv, int lane)
{
    if (nv <= 48) return hpr_reach(p, 1, nv);          // (every lane the same loop: broadcast reads)
    double m[9] = {0.0, -__builtin_inf(), -__builtin_inf(), -__builtin_inf(), -__builtin_inf(), -__builtin_inf(), -__builtin_inf(),
                   -__builtin_inf(), -__builtin_inf()};
    for (int k = lane; k < nv; k += kWave) {
        const double2 v = p[k];
        const double r2 = v.x * v.x + v.y * v.y, s = v.x + v.y, t = v.x - v.y;
        m[0] = r2 > m[0] ? r2 : m[0];
        m[1] = v.x > m[1] ? v.x : m[1];   m[2] = -v.x > m[2] ? -v.x : m[2];
        m[3] = v.y > m[3] ? v.y : m[3];   m[4] = -v.y > m[4] ? -v.y : m[4];
        m[5] = s > m[5] ? s : m[5];       m[8] = -s > m[8] ? -s : m[8];
        m[6] = t > m[6] ? t : m[6];       m[7] = -t > m[7] ? -t : m[7];
    }
#pragma unroll
    for (int q = 0; q < 9; q++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double other = __shfl_xor(m[q], o, kWave);
            m[q] = other > m[q] ? other : m[q];
        }
    }
    HprReach r;
    r.d2 = m[0]; r.xp = m[1]; r.xn = m[2]; r.yp = m[3]; r.yn = m[4]; r.pp = m[5]; r.pn = m[6]; r.np = m[7]; r.nn = m[8];
    return r;
}

// ---- decisions without the walk (wave-per-point pass) ----
// The points that reach the wave-per-point pass have met their nearest neighbours (home tiles); what is left of their
// polygons P is decided by very few of the remaining candidates, but the walk below finds those only by clipping with
// everything that still touches the polygon on the way (measured on 1024 x 10000: 50 - 90 clips for a point that ends
// hidden, every tile visited for one that ends visible: 19 k instructions per point).  So first, on a SCRATCH copy of P:
// take an interior point c, find the candidate whose constraint c violates MOST (one dot product per candidate, tiles
// culled for the single normal) -- none: c is strictly feasible with the verify margin, the point is visible -- else test
// whether that constraint (alone, or with one found earlier) excludes all of P, else clip the scratch polygon by it and
// repeat.  Both decisions are proofs about P, which is the exact path's own state, so they are what the walk would end
// with (below); anything undecided after kHprLpIters rounds takes the walk from P as before.  Measured on the CPU
// (tools/hpr_lp_study.py, scan / blob views): 99.7 % of the points decided, 1.2 - 1.4 rounds on average.
//   visible: the verify phase's argument (hpr_kernel), unchanged.
//   hidden: lam s1 + (1 - lam) s2 > m on every vertex of P for some lam in [0, 1] (s_i = a A_i + b B_i - C_i), hence on all
//     of P (affine).  Every vertex w the walk can still hold once it has taken both candidates satisfies s_i(w) <= eta, eta
//     = the walk's own rounding: a kept vertex has fl(s_i) <= 0, a crossing is computed on an edge inside P with a position
//     error of ~1e-16 of the edge's ends, later clips only take convex combinations of vertices that carry such errors
//     already; eta <= (12 + 3 G) u M after G clips, with M = the largest |a A_i| + |b B_i| + |C_i| over P's vertices (the
//     ends of those edges) and G <= n.  m = (1e-9 + 4e-15 n) M (at least ten times eta for any n, 10^4 times for the
//     tens of clips a walk really makes) therefore leaves the walk no vertex at all: it ends with the polygon empty,
//     whatever order it takes the candidates in and whichever of them it skips (it skips only candidates that cut nothing:
//     s_i <= 0 on all its vertices already).
constexpr int kHprLpIters = 4;
constexpr int kHprLpMaxV = 32;         // vertices of P (one per lane in the certificates); scratch polygons: 64

// an interior point of a convex polygon (every lane the same loop): the centroid; for a polygon that runs out to the
// box, a point near its bounded end (as the verify phase of hpr_kernel)
__device__ __forceinline__ bool hpr_interior(const double2 *src, int nv, double2 &c)
{
    double2 ctr = make_double2(0.0, 0.0), v0 = ctr, v1 = ctr;
    double r0 = __builtin_inf(), r1 = __builtin_inf();
    for (int k = 0; k < nv; k++) {
        const double2 v = src[k];
        const double r2 = v.x * v.x + v.y * v.y;
        ctr.x += v.x;
        ctr.y += v.y;
        if (r2 < r0) { r1 = r0; v1 = v0; r0 = r2; v0 = v; }
        else if (r2 < r1) { r1 = r2; v1 = v; }
    }
    ctr.x /= (double)nv;
    ctr.y /= (double)nv;
    if (!(ctr.x * ctr.x + ctr.y * ctr.y < 1.0e6)) {
        const double dx = ctr.x - v0.x, dy = ctr.y - v0.y;
        const double len = sqrt(dx * dx + dy * dy);
        double h = sqrt((v1.x - v0.x) * (v1.x - v0.x) + (v1.y - v0.y) * (v1.y - v0.y));
        h = h < 0.5 * len ? h : 0.5 * len;
        if (!(len > 0.0 && h > 0.0)) return false;
        ctr.x = v0.x + h * (dx / len);
        ctr.y = v0.y + h * (dy / len);
    }
    c = ctr;
    return ctr.x == ctr.x && ctr.y == ctr.y;
}

__device__ __forceinline__ double hpr_wave_max(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double other = __shfl_xor(v, o, kWave);
        v = other > v ? other : v;
    }
    return v;
}

// does the constraint (A, B, C) alone, or some mix of it with (A1, B1, C1), exclude every vertex of P by the margin?
// (lane k holds vertex k; nv <= kHprLpMaxV)
__device__ __forceinline__ bool hpr_excluded(const double2 *P, int nv, bool pair, double A1, double B1, double C1, double A, double B,
                                             double C, int lane, double margin)
{
    const bool mine = lane < nv;
    const double2 v = mine ? P[lane] : make_double2(0.0, 0.0);
    const double s2 = v.x * A + v.y * B - C, M2 = fabs(v.x * A) + fabs(v.y * B) + fabs(C);
    const double s1 = pair ? v.x * A1 + v.y * B1 - C1 : 0.0, M1 = pair ? fabs(v.x * A1) + fabs(v.y * B1) + fabs(C1) : 0.0;
    const double m = margin * hpr_wave_max(mine ? (M1 > M2 ? M1 : M2) : 0.0);
    if (!(m < __builtin_inf())) return false;
    if (__ballot(mine && !(s2 > m)) == 0ull) return true;            // the new constraint alone
    if (!pair) return false;
    // lam s1 + (1 - lam) s2 > m  <=>  s2 + lam (s1 - s2) > m: an interval of lam per vertex
    double lo = 0.0, hi = 1.0;
    if (mine) {
        const double d = s1 - s2;
        if (d > 0.0) lo = (m - s2) / d;
        else if (d < 0.0) hi = (m - s2) / d;
        else if (!(s2 > m)) lo = 2.0;
    }
    lo = hpr_wave_max(lo);
    hi = -hpr_wave_max(-hi);
    lo = lo > 0.0 ? lo : 0.0;
    hi = hi < 1.0 ? hi : 1.0;
    if (!(lo < hi)) return false;
    const double lam = 0.5 * (lo + hi);
    const double g = lam * s1 + (1.0 - lam) * s2;          // the certificate itself, evaluated as such
    return __ballot(mine && !(g > m)) == 0ull;
}

// One point's decision rounds (see above): P = its polygon as the exact path left it (nv <= kHprLpMaxV vertices), scratch =
// room for two polygons of 64 vertices.  -> 0 undecided, 1 visible, 2 hidden.
__device__ __forceinline__ int hpr_decide(const HprFrame &f, const double2 *P, int nv, double2 *scratch, const double *__restrict__ fl,
                                          int n, int ntiles, const HprTile *__restrict__ tiles, int home, int pos, int lane)
{
    // the hidden proof's margin, relative to M (above): the walk's rounding grows with the clips behind a vertex -- a vertex
    // made by the G-th clip sits on an edge whose ends carry (12 + 3 (G - 1)) u M already -- and G <= n
    const double margin = 1e-9 + 4e-15 * (double)n;
    const double2 *poly = P;
    int pn = nv, nprev = 0;
    double pA[kHprLpIters], pB[kHprLpIters], pC[kHprLpIters];
    for (int it = 0; it < kHprLpIters; it++) {
        double2 c;
        if (!hpr_interior(poly, pn, c)) break;
        const double nx = f.ux + c.x * f.e1x + c.y * f.e2x, ny = f.uy + c.x * f.e1y + c.y * f.e2y,
                     nz = f.uz + c.x * f.e1z + c.y * f.e2z;
        const double nn = 1.0 + c.x * c.x + c.y * c.y;
        const double thr = 1e-10 * f.rho * nn;
        const double cl = sqrt(nn) * (1.0 + 1e-15), cpsi1 = 1.0 / cl, spsi1 = sqrt(nn - 1.0) / cl * (1.0 + 1e-15);
        // the candidate c violates most (distance to its line); key < 0: none comes within the margin
        double key = -1.0, kA = 0.0, kB = 0.0, kC = 0.0;
        int kj = INT_MAX;
        // Tiles outward from the point's own: what hides a point is near it in direction, and the first candidate found
        // to exclude all of P ends the scan (two thirds of the parked points end hidden) -- so the own tile and its two
        // neighbours are taken before any tile record is looked at.  Two tiles at a time (twelve loads in flight: this
        // loop waits on memory).  A lane tests only its most violated candidate so far for exclusion, once per pair.
        auto scan_pair = [&](int ta, int tb) -> bool {
            constexpr int kPer = kHprThreads / kWave;
            double q[2 * kPer][3];
            int jj[2 * kPer];
#pragma unroll
            for (int e = 0; e < 2 * kPer; e++) {
                const int tile = e < kPer ? ta : tb;
                const int j = tile * kHprThreads + (e % kPer) * kWave + lane;
                jj[e] = (tile >= 0 && j < n) ? j : -1;
                const int jl = jj[e] >= 0 ? j : pos;           // (a harmless address: the point itself)
                q[e][0] = fl[(size_t)jl * 3 + 0];
                q[e][1] = fl[(size_t)jl * 3 + 1];
                q[e][2] = fl[(size_t)jl * 3 + 2];
            }
            bool fresh = false;
#pragma unroll
            for (int e = 0; e < 2 * kPer; e++) {
                const double qx = q[e][0], qy = q[e][1], qz = q[e][2];
                // (a sieve with the verify margin behind it: fused multiply-adds, and the point itself recognised by its
                // position -- what passes is valued below with the walk's own operations)
                const double sv = __builtin_fma(nz, qz, __builtin_fma(ny, qy, nx * qx)) - f.rho;
                if (jj[e] >= 0 && jj[e] != pos && sv > -thr) {           // (NaN rows: false)
                    const double A = f.e1x * qx + f.e1y * qy + f.e1z * qz;
                    const double B = f.e2x * qx + f.e2y * qy + f.e2z * qz;
                    const double l2 = A * A + B * B;
                    const double k2 = sv > 0.0 ? (l2 > 0.0 ? sv * sv / l2 : __builtin_inf()) : 0.0;
                    if (k2 > key || (k2 == key && jj[e] < kj)) {
                        key = k2; kj = jj[e]; kA = A; kB = B;
                        kC = f.rho - (f.ux * qx + f.uy * qy + f.uz * qz);
                        fresh = true;
                    }
                }
            }
            // does the lane's candidate alone exclude all of P (hpr_excluded's test, a lane per candidate)?
            bool excl = false;
            if (fresh) {
                double smin = __builtin_inf(), mmax = 0.0;
                for (int k = 0; k < nv; k++) {
                    const double2 v = P[k];
                    const double sk = v.x * kA + v.y * kB - kC, mk = fabs(v.x * kA) + fabs(v.y * kB) + fabs(kC);
                    smin = sk < smin ? sk : smin;
                    mmax = mk > mmax ? mk : mmax;
                }
                excl = mmax < __builtin_inf() && smin > margin * mmax;
            }
            return __ballot(excl) != 0ull;
        };
        for (int ph = 0, t0 = 0; t0 < 2 * ntiles;) {
            const int tl = hpr_tile_of(t0 + lane, home);
            bool need = tl >= 0 && tl < ntiles;
            if (ph == 0) need = need && lane < 3;          // the own tile and its neighbours: no questions asked
            else need = need && t0 + lane >= 3 && hpr_tile_needed(f, cpsi1, spsi1, &c, 0, 1, tiles[tl]);
            unsigned long long todo = __ballot(need);
            while (todo) {
                const int b0 = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                int b1 = -1;
                if (todo) {
                    b1 = __ffsll((long long)todo) - 1;
                    todo &= todo - 1;
                }
                if (scan_pair(hpr_tile_of(t0 + b0, home), b1 >= 0 ? hpr_tile_of(t0 + b1, home) : -1)) return 2;
            }
            if (ph == 0) ph = 1;
            else t0 += kWave;
        }
        double bkey = key;
        int bj = kj;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ok = __shfl_xor(bkey, o, kWave);
            const int oj = __shfl_xor(bj, o, kWave);
            if (ok > bkey || (ok == bkey && oj < bj)) { bkey = ok; bj = oj; }
        }
        if (bkey < 0.0) return 1;                 // c is strictly feasible: visible
        const int owner = __ffsll((long long)__ballot(kj == bj && key == bkey)) - 1;
        const double A = __shfl(kA, owner, kWave), B = __shfl(kB, owner, kWave), C = __shfl(kC, owner, kWave);
        bool hidden = hpr_excluded(P, nv, false, 0.0, 0.0, 0.0, A, B, C, lane, margin);
#pragma unroll
        for (int q = kHprLpIters - 2; q >= 0; q--)
            if (q < nprev && !hidden) hidden = hpr_excluded(P, nv, true, pA[q], pB[q], pC[q], A, B, C, lane, margin);
        if (hidden) return 2;
        if (it + 1 == kHprLpIters) break;
        double2 *dst = scratch + (it & 1) * 64;
        const int m = hpr_clip_wave(poly, pn, A, B, C, dst, lane);
        __syncthreads();
        if (m < 3 || m > 62) break;
        poly = dst;
        pn = m;
#pragma unroll
        for (int q = 0; q < kHprLpIters - 1; q++)
            if (q == nprev) { pA[q] = A; pB[q] = B; pC[q] = C; }
        nprev++;
    }
    return 0;
}

// The parked points' first try in a kernel of its own: the rounds above wait on memory (a wave lives ~20 us, most of it
// in a dozen dependent round trips), so what matters is how many waves a CU holds -- this kernel needs a third of the
// registers of hpr_overflow_kernel, whose walk and clip code the 98 % of the points decided here never run.  Undecided
// points (and the ones that still have home tiles to take after the try) are listed for hpr_overflow_kernel by slot.
__device__ __forceinline__ void hpr_decide_item(int slot, int n, const double *__restrict__ fl_all, const HprTile *__restrict__ tiles_all,
                                                unsigned char *__restrict__ vis, int *__restrict__ cnt, int *status,
                                                const int *__restrict__ perm, const unsigned char *__restrict__ alive,
                                                const int4 *__restrict__ surv, const double2 *__restrict__ surv_poly,
                                                int *__restrict__ slots, const HprSegs &segs, double2 *s_p, double2 *s_scratch)
{
    const int lane = threadIdx.x;
    const int4 rec = surv[slot];
    const int view = rec.x / n, nv = rec.y, pos = rec.z;
    if (alive && !alive[view]) return;        // (wave-uniform) a view that cannot be the best any more
    const int i = perm[(size_t)view * n + pos];
    const double *fl = fl_all + (size_t)view * n * 3;
    const int ntiles = ceil_div_dev(n, kHprThreads);
    HprFrame f;
    if (!hpr_frame(fl + (size_t)pos * 3, f)) return;
    if (lane < nv) s_p[lane] = surv_poly[(size_t)slot * kHprMaxV + lane];
    __syncthreads();
    int d = 0;
    if (nv >= 3) d = hpr_decide(f, s_p, nv, s_scratch, fl, n, ntiles, tiles_all + (size_t)view * ntiles, pos / kHprThreads, pos, lane);
    if (lane == 0) {
        if (d) {
            vis[(size_t)view * n + i] = d == 1 ? 1 : 0;
            if (d == 1) atomicAdd(&cnt[view], 1);
        } else {
            slots[atomicAdd(&status[kHprStUndecided], 1)] = slot;
        }
    }
}

// The launch does not know how many points were parked (the count never leaves the device): a fixed grid of one-wave
// blocks, a multiple of 8 of them, strides over the items -- block b stays with segment b % 8, the XCD it runs on.
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(3, 8))) void hpr_decide_kernel(int n, const double *__restrict__ fl_all, const HprTile *__restrict__ tiles_all,
                                                          unsigned char *__restrict__ vis, int *__restrict__ cnt, int *status,
                                                          const int *__restrict__ perm, const unsigned char *__restrict__ alive,
                                                          const int4 *__restrict__ surv, const double2 *__restrict__ surv_poly,
                                                          int *__restrict__ slots, const HprSegs *__restrict__ segs_p, int *work)
{
    __shared__ double2 s_p[kHprMaxV + 6];
    __shared__ double2 s_scratch[128];
    const HprSegs segs = *segs_p;
    // this block's segment, its first slot and its fill (wave-uniform: the loop stays scalar)
    const int x = segs.on ? (int)(blockIdx.x & 7) : 0, stride = segs.on ? (int)(gridDim.x >> 3) : (int)gridDim.x;
    const int first = segs.base[x];
    const int fill = __builtin_amdgcn_readfirstlane(min(status[kHprStSegFill + x], segs.cap - first));
    // The first chunk of kHprDecideChunk consecutive points is the block's own; the following ones are drawn from the
    // segment's counter in order of arrival, so that the waves in flight work on a narrow window of the segment -- a few
    // views' flipped points and tile records in that XCD's L2, as when every item was a block of its own and the dispatcher
    // handed them out in order.  (A fixed stride lets the waves drift apart over hundreds of views: 9.2 ms against 6.7 at
    // 1024 x 10000; a draw per POINT from eight counters in one cache line serialised the launch: 18.8 ms -- the counters
    // have a 128-byte line each and a draw covers four points.)
    int k0 = (segs.on ? (int)(blockIdx.x >> 3) : (int)blockIdx.x) * kHprDecideChunk;
    while (k0 < fill) {
        int nxt = 0;
        if (threadIdx.x == 0) nxt = atomicAdd(&work[(kHprWorkFirstTry + x) * kHprWorkLine], 1);          // (issued now, read after the chunk)
        for (int k = k0; k < min(k0 + kHprDecideChunk, fill); k++) {
            hpr_decide_item(first + k, n, fl_all, tiles_all, vis, cnt, status, perm, alive, surv, surv_poly, slots, segs, s_p, s_scratch);
            __syncthreads();
        }
        k0 = (stride + __builtin_amdgcn_readfirstlane(nxt)) * kHprDecideChunk;
    }
}

// CAP = vertices a polygon may reach: the pass runs with 128 first (4 KiB of LDS per wave: forty waves per CU instead
// of the five that two 16 KiB buffers allow) and hands the few polygons that outgrow that to a second launch with
// kHprOverCap (list2, counted in status[kHprStOver128]); results do not depend on the tier.
template <int CAP>
__device__ __forceinline__ void hpr_overflow_item(int item, int n, const double *__restrict__ fl_all,
                                                  const HprTile *__restrict__ tiles_all, unsigned char *__restrict__ vis,
                                                  int *__restrict__ cnt, int *status, const int *__restrict__ list,
                                                  const int *__restrict__ perm, const int *__restrict__ hardlist,
                                                  const int *__restrict__ hardcnt, int no_cull,
                                                  const unsigned char *__restrict__ alive, int *__restrict__ list2,
                                                  const int4 *__restrict__ surv, const double2 *__restrict__ surv_poly,
                                                  double2 *__restrict__ gbuf, int gcap, const int *__restrict__ slots, const HprSegs &segs,
                                                  double2 (*s_lds)[CAP > 0 ? CAP : 1])
{
    // CAP == 0: the polygon lives in global memory, gcap vertices per buffer (n + 8: a polygon has at most one edge per
    // other point and four of the box -- this tier cannot overflow; round 3 returned an error beyond 1024 vertices)
    double2 *s_buf[2];
    s_buf[0] = CAP > 0 ? s_lds[0] : gbuf + (size_t)blockIdx.x * 2 * gcap;          // (a pair of buffers per BLOCK)
    s_buf[1] = CAP > 0 ? s_lds[1] : gbuf + ((size_t)blockIdx.x * 2 + 1) * gcap;
    const int cap = CAP > 0 ? CAP : gcap;
    const int lane = threadIdx.x;
    // surv != null: the points the split first kernel left undecided continue HERE from their saved polygons (home tiles and
    // verification are behind them), one wave each
    const bool cont = surv != nullptr;
    // (a parked point's record carries its position: one dependent load less in front of the first useful one)
    // (slots: the parked points hpr_decide_kernel left undecided -- their first try is behind them)
    const int slot = !cont ? 0 : (slots ? slots[item] : hpr_seg_slot(segs, status, item));
    if (slot < 0) return;
    const int4 rec = cont ? surv[slot] : make_int4(list[item], 4, -1, 0);
    const int id = rec.x, view = id / n, rank = id - view * n;
    if (alive && !alive[view]) return;        // (wave-uniform) a view that cannot be the best any more
    const int *hl = hardlist + (size_t)view * n;
    const int pos = cont ? rec.z : hl[rank], i = perm[(size_t)view * n + pos];
    const double *fl = fl_all + (size_t)view * n * 3;
    const int ntiles = ceil_div_dev(n, kHprThreads);
    const HprTile *tiles = tiles_all + (size_t)view * ntiles;
    HprFrame f;
    if (!hpr_frame(fl + (size_t)pos * 3, f)) return;      // (cannot happen: the first pass listed it)
    int cur = 0, nv = 4;
    // home tiles the exact path has behind it (0 .. 3) and candidates of the next one already taken (hpr_kernel's park)
    const int rel0 = cont ? rec.w >> 8 : 0, skip0 = cont ? rec.w & 255 : 0;
    if (cont) {
        nv = rec.y;
        if (lane < nv) s_buf[0][lane] = surv_poly[(size_t)slot * kHprMaxV + lane];
    } else if (lane == 0) {
        s_buf[0][0] = make_double2(-kHprBox, -kHprBox);
        s_buf[0][1] = make_double2(kHprBox, -kHprBox);
        s_buf[0][2] = make_double2(kHprBox, kHprBox);
        s_buf[0][3] = make_double2(-kHprBox, kHprBox);
    }
    __syncthreads();
    HprReach R = hpr_reach(s_buf[0], 1, nv);
    bool failed = false;
    const int home = pos / kHprThreads;
    // one tile of candidates against the polygon (32 candidates at a time)
    auto take_tile = [&](int tile, int skip) {
        const int tile0 = tile * kHprThreads;
            // the first pass's order: 32-candidate chunks, in the home tile starting with the point's own
            // (any other tile is taken in ascending order: 64 candidates at a time there)
            const bool is_home = tile == home;
            const int rot = is_home ? ((pos - home * kHprThreads) >> 5) : 0;
            const int width = is_home ? 32 : kWave;
            for (int cc = 0; cc < kHprThreads / width && nv > 0; cc++) {
                if ((cc + 1) * width <= skip) continue;              // (taken before the point was parked)
                const int j = tile0 + (is_home ? ((cc + rot) & (kHprThreads / 32 - 1)) * 32 : cc * kWave) + lane;
                double A = 0.0, B = 0.0, C = 0.0;
                bool pass = false;
                if (lane < width && cc * width + lane >= skip && j < n) {
                    const double qx = fl[(size_t)j * 3 + 0], qy = fl[(size_t)j * 3 + 1], qz = fl[(size_t)j * 3 + 2];
                    A = f.e1x * qx + f.e1y * qy + f.e1z * qz;
                    B = f.e2x * qx + f.e2y * qy + f.e2z * qz;
                    C = f.rho - (f.ux * qx + f.uy * qy + f.uz * qz);
                    const bool self = qx == f.px && qy == f.py && qz == f.pz;
                    pass = !self && qx == qx && !hpr_far(R, A, B, C);
                }
                // every lane tests ITS candidate against the whole polygon (broadcast reads); only the ones
                // that cut anything are then taken one by one (a candidate that does not cut the polygon now
                // cannot cut what is left of it later) -- the tail of this kernel is a point with 20000
                // candidates in reach of its polygon of which 1400 cut: 29 ms when each was taken serially
                if (pass) {
                    const double2 *pv = s_buf[cur];
                    bool cuts = false;
                    for (int k = 0; k < nv; k++) cuts |= pv[k].x * A + pv[k].y * B - C > 0.0;
                    pass = cuts;
                }
                unsigned long long mask = __ballot(pass);
                bool clipped = false;
                while (mask && nv > 0) {
                    const int from = __ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    const double Aj = __shfl(A, from, kWave), Bj = __shfl(B, from, kWave), Cj = __shfl(C, from, kWave);
                    const double2 *src = s_buf[cur];
                    int out = 0;
                    for (int k = lane; k < nv; k += kWave) out += (src[k].x * Aj + src[k].y * Bj - Cj > 0.0) ? 1 : 0;
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) out += __shfl_xor(out, o, kWave);
                    if (!out) continue;
                    if (out == nv) { nv = 0; break; }
                    if (nv - out + 2 > cap) {
                        if (lane == 0) {
                            if (CAP > 0 && CAP < kHprOverCap) list2[atomicAdd(&status[kHprStOver128], 1)] = id;      // the large-polygon launch takes it
                            else if (CAP == kHprOverCap) list2[atomicAdd(&status[kHprStOverCap], 1)] = id;          // the global-memory tier takes it
                            else atomicExch(&status[kHprStError], 2);                                            // (cannot happen: gcap = n + 8)
                        }
                        failed = true;
                        nv = 0;
                        break;
                    }
                    const int m = hpr_clip_wave(src, nv, Aj, Bj, Cj, s_buf[cur ^ 1], lane);
                    __syncthreads();
                    if (m < 3) { nv = 0; break; }
                    nv = m;
                    cur ^= 1;
                    clipped = true;
                }
                // (the reach bounds only feed conservative rejections, and a clip only shrinks the polygon: refreshed once
                // per 64 candidates instead of after every clip -- half the instructions of a clip; the slowest walker,
                // 1400 clips, is what the launch waits for)
                if (clipped && nv > 0) R = hpr_reach_wave(s_buf[cur], nv, lane);
            }
    };
    bool lp_ran = false;
    // -> 0 undecided, 1 visible, 2 hidden
    auto lp_try = [&]() -> int {
        if (!(CAP >= 128 && nv >= 3 && nv <= kHprLpMaxV && !(no_cull & kHprNoRounds))) return 0;
        lp_ran = true;
        const int d = hpr_decide(f, s_buf[cur], nv, s_buf[cur ^ 1], fl, n, ntiles, tiles, home, pos, lane);
        if (d) return d;
        __syncthreads();          // (the walk reuses the scratch buffer)
        return 0;
    };
    auto decided = [&](int d) {
        if (lane == 0) {
            vis[(size_t)view * n + i] = d == 1 ? 1 : 0;
            if (d == 1) atomicAdd(&cnt[view], 1);
        }
    };
    // the first pass's order: the home tile and its neighbours, then outward from the group's tile.  A parked point is
    // tried before its remaining home tiles are taken (most are decided from the polygon they bring), and again after.
    if (cont && rel0 < 3 && !slots) {
        const int d = lp_try();
        if (d) { decided(d); return; }
    }
    for (int rel = rel0; rel < 3 && nv > 0; rel++) {
        const int tile = home + (rel == 0 ? 0 : (rel == 1 ? 1 : -1));
        if (tile >= 0 && tile < ntiles) take_tile(tile, rel == rel0 ? skip0 : 0);
    }
    if (!(slots && rel0 >= 3)) {
        const int d = lp_try();
        if (d) { decided(d); return; }
    }
    if (nv >= 3 && !cont && !lp_ran) {
        const double2 *src = s_buf[cur];
        double2 ctr = make_double2(0.0, 0.0), v0 = ctr, v1 = ctr;
        double r0 = __builtin_inf(), r1 = __builtin_inf();
        for (int k = 0; k < nv; k++) {
            const double2 v = src[k];
            const double r2 = v.x * v.x + v.y * v.y;
            ctr.x += v.x;
            ctr.y += v.y;
            if (r2 < r0) { r1 = r0; v1 = v0; r0 = r2; v0 = v; }
            else if (r2 < r1) { r1 = r2; v1 = v; }
        }
        ctr.x /= (double)nv;
        ctr.y /= (double)nv;
        const bool open = !(ctr.x * ctr.x + ctr.y * ctr.y < 1.0e6);
        const double dx = ctr.x - v0.x, dy = ctr.y - v0.y;
        const double len = sqrt(dx * dx + dy * dy);
        double h = sqrt((v1.x - v0.x) * (v1.x - v0.x) + (v1.y - v0.y) * (v1.y - v0.y));
        h = h < 0.5 * len ? h : 0.5 * len;
        for (int trial = 0; trial < (open ? 4 : 1); trial++) {
            double2 c = ctr;
            if (open) {
                if (!(len > 0.0 && h > 0.0)) break;
                c.x = v0.x + h * (dx / len);
                c.y = v0.y + h * (dy / len);
                h *= 0.125;
            }
            const double nx = f.ux + c.x * f.e1x + c.y * f.e2x, ny = f.uy + c.x * f.e1y + c.y * f.e2y,
                         nz = f.uz + c.x * f.e1z + c.y * f.e2z;
            const double thr = 1e-10 * f.rho * (1.0 + c.x * c.x + c.y * c.y);
            bool bad = false;
            for (int j0 = 0; j0 < n && !bad; j0 += kWave) {
                const int j = j0 + lane;
                bool b1 = false;
                if (j < n) {
                    const double qx = fl[(size_t)j * 3 + 0], qy = fl[(size_t)j * 3 + 1], qz = fl[(size_t)j * 3 + 2];
                    const double sv = (nx * qx + ny * qy + nz * qz) - f.rho;
                    const bool self = qx == f.px && qy == f.py && qz == f.pz;
                    b1 = !self && sv > -thr;
                }
                bad = __ballot(b1) != 0ull;
            }
            if (!bad) {
                if (lane == 0) {
                    vis[(size_t)view * n + i] = 1;
                    atomicAdd(&cnt[view], 1);
                }
                return;
            }
        }
    }
    const int own = hpr_base_tile(hl, hardcnt[view], rank);
    [[maybe_unused]] const unsigned long long walk_t0 = HPR_PROF_CLOCK();
    [[maybe_unused]] const int walk_nv0 = nv;
    [[maybe_unused]] const double walk_d2 = R.d2;
    for (int step0 = 0, bsz = 1; step0 < 2 * ntiles && nv > 0; step0 += bsz, bsz = step0 < kWave ? step0 : kWave) {
        bool need = false;
        if (lane < bsz) {
            const int tile = hpr_tile_of(step0 + lane, own);
            const double l = sqrt(1.0 + R.d2) * (1.0 + 1e-15), cpsi = 1.0 / l, spsi = sqrt(R.d2) / l * (1.0 + 1e-15);
            if (tile >= 0 && tile < ntiles && !(tile >= home - 1 && tile <= home + 1))
                need = hpr_tile_needed(f, cpsi, spsi, s_buf[cur], 1, nv, tiles[tile]);
        }
        unsigned long long todo = __ballot(need);
        while (todo && nv > 0) {
            const int b = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            take_tile(hpr_tile_of(step0 + b, own), 0);
        }
    }
#ifdef GENPC_HPR_PROF
    if (lane == 0 && walk_nv0 > 0) {
        const unsigned long long dt = HPR_PROF_CLOCK() - walk_t0;
        atomicAdd(&g_hpr_prof[10], 1ull);                       // walkers
        atomicAdd(&g_hpr_prof[11], dt);                         // their ticks
        atomicMax(&g_hpr_prof[12], dt);                         // the slowest
        if (dt > 200000ull) atomicAdd(&g_hpr_prof[13], 1ull);   // walkers over 100 us
        if (walk_d2 > 1.0e6) { atomicAdd(&g_hpr_prof[14], 1ull); atomicAdd(&g_hpr_prof[15], dt); }      // open polygons: count, ticks
        if (dt > 200000ull && nv > 0) atomicAdd(&g_hpr_prof[9], 1ull);      // slow walkers that end visible
    }
#endif
    if (failed) return;
    if (lane == 0) {
        vis[(size_t)view * n + i] = nv > 0 ? 1 : 0;
        if (nv > 0) atomicAdd(&cnt[view], 1);
    }
}

// A fixed grid of one-wave blocks over a count that lives on the device (`count`: a word of status; null: the parked
// points by segment).  A wave's first item is its block index, the following ones it draws from `work` (zero at launch) --
// walkers take from 10 us to over a millisecond, so the items are handed out as waves come free; the draw is issued
// before the item is worked on and read after it.
template <int CAP>
__global__ __launch_bounds__(kWave) void hpr_overflow_kernel(int n, const double *__restrict__ fl_all,
                                                             const HprTile *__restrict__ tiles_all, unsigned char *__restrict__ vis,
                                                             int *__restrict__ cnt, int *status, const int *__restrict__ list,
                                                             const int *__restrict__ perm, const int *__restrict__ hardlist,
                                                             const int *__restrict__ hardcnt, int no_cull,
                                                             const unsigned char *__restrict__ alive, int *__restrict__ list2,
                                                             const int4 *__restrict__ surv, const double2 *__restrict__ surv_poly,
                                                             double2 *__restrict__ gbuf, int gcap, const int *__restrict__ slots,
                                                             const HprSegs *__restrict__ segs_p, const int *count, int *work)
{
    // (work: this pass's counter, a line of its own)
    __shared__ double2 s_lds[2][CAP > 0 ? CAP : 1];
    const HprSegs segs = *segs_p;
    const int items = __builtin_amdgcn_readfirstlane(count ? *count : hpr_seg_items(segs, status));
    int item = blockIdx.x;
    while (item < items) {
        int nxt = 0;
        if (threadIdx.x == 0) nxt = atomicAdd(work, 1);
        hpr_overflow_item<CAP>(item, n, fl_all, tiles_all, vis, cnt, status, list, perm, hardlist, hardcnt, no_cull, alive, list2, surv,
                               surv_poly, gbuf, gcap, slots, segs, s_lds);
        __syncthreads();
        item = (int)gridDim.x + __builtin_amdgcn_readfirstlane(nxt);          // (lane 0's draw)
    }
}

// One launch of the walk: `list` (null: the parked points, by `slots` or by segment) counted in status word `count`
// (< 0: by segment), polygons that outgrow the tier go to `list2`
template <int CAP>
static bool launch_walk(const HprCall &k, int blocks, hipStream_t stream, const int *list, int *list2, bool parked, const int *slots, int count,
                        int work_line, int gcap, const char *what)
{
    hipLaunchKernelGGL(hpr_overflow_kernel<CAP>, dim3(blocks), dim3(kWave), 0, stream, k.n, (const double *)k.fl, (const HprTile *)k.tiles, k.visible,
                       k.counts, k.status, list, (const int *)k.i1, (const int *)k.hardlist, (const int *)k.hardcnt, k.no_cull,
                       (const unsigned char *)k.alive, list2, parked ? (const int4 *)k.surv : (const int4 *)nullptr,
                       parked ? (const double2 *)k.surv_poly : (const double2 *)nullptr, CAP > 0 ? (double2 *)nullptr : k.gbuf, gcap, slots,
                       (const HprSegs *)k.segs(), count >= 0 ? (const int *)(k.status + count) : (const int *)nullptr, k.work + work_line * kHprWorkLine);
    return check(hipGetLastError(), what);
}

bool hpr_launch_wave(const HprPlan &plan, const HprCall &k, hipStream_t stream)
{
    int *list2 = (int *)k.k0;          // (the sort's key buffer is free by now; at most views x points entries)
    int *list3 = (int *)k.k1;          // (likewise: the points whose polygons outgrow the 1024-vertex tier)
    if (plan.split) {
        const int *slots = nullptr;
        int count = -1;                // (the parked points by segment)
        if (plan.decide_kernel) {
            int *sl = k.i0;            // (the sort's index buffer is free by now; at most views x points entries)
            hipLaunchKernelGGL(hpr_decide_kernel, dim3(plan.decide_blocks), dim3(kWave), 0, stream, k.n, (const double *)k.fl, (const HprTile *)k.tiles,
                               k.visible, k.counts, k.status, (const int *)k.i1, (const unsigned char *)k.alive, (const int4 *)k.surv,
                               (const double2 *)k.surv_poly, sl, (const HprSegs *)k.segs(), k.work);
            if (!check(hipGetLastError(), "hpr decide launch")) return false;
            slots = sl;
            count = kHprStUndecided;
        }
        if (!launch_walk<128>(k, plan.walk_blocks, stream, nullptr, list2, true, slots, count, kHprWorkContinue, 0, "hpr continuation launch")) return false;
    }
    if (!launch_walk<128>(k, plan.walk_blocks, stream, k.list, list2, false, nullptr, kHprStListed, kHprWorkListed, 0, "hpr second pass launch")) return false;
    // polygons over 128 vertices (from the two launches above)
    if (!launch_walk<kHprOverCap>(k, plan.large_blocks, stream, list2, list3, false, nullptr, kHprStOver128, kHprWorkLarge, 0, "hpr large-polygon launch")) return false;
    // polygons over 1024 vertices: the polygon in global memory, it cannot overflow
    if (!launch_walk<0>(k, plan.global_blocks, stream, list3, nullptr, false, nullptr, kHprStOverCap, kHprWorkGlobal, plan.gcap, "hpr global-polygon launch")) return false;
    hipLaunchKernelGGL(hpr_finish_kernel, dim3(plan.view_grid), dim3(256), 0, stream, k.c, (const int *)k.status, k.counts);
    return true;
}

}  // namespace genpc
