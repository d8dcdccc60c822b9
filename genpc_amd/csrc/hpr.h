// hpr.h -- what the hidden-point-removal files share (hpr.hip: the call; hpr_order.hip, hpr_accept.hip, hpr_first.hip,
// hpr_wave.hip: its passes): the records, the device helpers every pass uses, the status header's words, the work
// counters' lines and the launchers.  The algorithm is described at the head of hpr.hip, the plan of a call in hpr_plan.h.
#pragma once
#pragma clang fp contract(off)
#include "common.h"
#include "hpr_plan.h"

namespace genpc {

constexpr double kHprBox = 1.0e4;

// The 256-byte status header, hand-placed and to stay so (zeroed per call; the bounds then set to 0xff): counters the
// passes read their item counts from, the cloud's bounds, the segments' fills and the segment record.
enum HprStatus : int {
    kHprStListed = 0,          // points handed to the wave-per-point pass (they restart from the box)
    kHprStError = 1,           // 2: a polygon outgrew its buffer (every count becomes -1)
    kHprStParked = 2,          // points the split first kernel parked with their polygons
    kHprStOver128 = 3,         // polygons over 128 vertices: the large-polygon launch's
    kHprStOverCap = 4,         // polygons over kHprOverCap vertices: the global-memory tier's
    kHprStUndecided = 5,       // parked points the first try left undecided
    kHprStBounds = 16,         // min[3], max[3] of the finite coordinates as ordered uints
    kHprStSegFill = 32,        // [x]: parked points of segment x
    kHprStSegs = 48,           // HprSegs
};
// The work counters of the wave-per-point passes: line k is the ints from k * kHprWorkLine
enum HprWork : int {
    kHprWorkFirstTry = 0,      // eight lines, one per segment
    kHprWorkContinue = 8,      // the parked points' continuation
    kHprWorkListed = 9,
    kHprWorkLarge = 10,
    kHprWorkGlobal = 11,
};

__device__ __forceinline__ unsigned hpr_ord(float f)      // order-preserving float -> uint
{
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float hpr_unord(unsigned o)
{
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// The frame in which a view's directions are ordered: w = towards the centre of the cloud's bounding box,
// (E1, E2) the completion hpr_frame uses, s = the largest |x|, |y| a direction to a point of the box can have
// (sine of the bounding sphere's angular radius, 5 % slack; 1 when the eye is inside that sphere).
struct HprViewFrame {
    double e1x, e1y, e1z, e2x, e2y, e2z, s;
};

__device__ __forceinline__ int ceil_div_dev(int a, int b) { return (a + b - 1) / b; }

struct HprFrame {
    double px, py, pz, rho, ux, uy, uz, e1x, e1y, e1z, e2x, e2y, e2z;
};

// u, e1, e2 of a flipped point; false when it coincides with the origin or is not finite
__device__ __forceinline__ bool hpr_frame(const double *p, HprFrame &f)
{
    f.px = p[0]; f.py = p[1]; f.pz = p[2];
    f.rho = sqrt(f.px * f.px + f.py * f.py + f.pz * f.pz);
    if (!(f.rho > 0.0) || !(f.rho < __builtin_inf())) return false;
    f.ux = f.px / f.rho; f.uy = f.py / f.rho; f.uz = f.pz / f.rho;
    const double ax = fabs(f.ux), ay = fabs(f.uy), az = fabs(f.uz);
    double x, y, z;
    if (ax <= ay && ax <= az) { x = 0.0; y = f.uz; z = -f.uy; }
    else if (ay <= az)        { x = -f.uz; y = 0.0; z = f.ux; }
    else                      { x = f.uy; y = -f.ux; z = 0.0; }
    const double l = sqrt(x * x + y * y + z * z);
    f.e1x = x / l; f.e1y = y / l; f.e1z = z / l;
    f.e2x = f.uy * f.e1z - f.uz * f.e1y;
    f.e2y = f.uz * f.e1x - f.ux * f.e1z;
    f.e2z = f.ux * f.e1y - f.uy * f.e1x;
    return true;
}

// What a thread needs to know about a tile of kHprThreads consecutive (Morton-neighbour) candidates to skip
// it whole: their directions lie within angle phi of the axis w, their lengths are <= rho_max.
struct HprTile {
    double wx, wy, wz, cos_phi, sin_phi, cos2_phi, sin2_phi, inv_rho_max;
};

// Sutherland-Hodgman against a A + b B <= C: src (nv vertices, element k at src[k * ss]) -> dst (stride ds);
// returns the new count.  A vertex exactly on the line is kept and spawns no intersection point.
__device__ __forceinline__ int hpr_clip(const double2 *src, int ss, int nv, double A, double B, double C, double2 *dst, int ds)
{
    int m = 0;
    double2 cur = src[0];
    double s0 = cur.x * A + cur.y * B - C;
    for (int k = 0; k < nv; k++) {
        const int k2 = k + 1 < nv ? k + 1 : 0;
        const double2 nxt = src[(size_t)k2 * ss];
        const double s1 = nxt.x * A + nxt.y * B - C;
        if (!(s0 > 0.0)) dst[(size_t)(m++) * ds] = cur;
        if ((s0 > 0.0) != (s1 > 0.0) && s0 != 0.0 && s1 != 0.0) {
            const double t = s0 / (s0 - s1);
            double2 x;
            x.x = cur.x + t * (nxt.x - cur.x);
            x.y = cur.y + t * (nxt.y - cur.y);
            dst[(size_t)(m++) * ds] = x;
        }
        cur = nxt;
        s0 = s1;
    }
    return m;
}

// The same clip IN PLACE (no scratch): the outside vertices of a convex polygon are one cyclic run [f, f+L);
// it is replaced by the two edge crossings.  Each crossing is computed exactly as hpr_clip does (from the
// edge's first vertex, in the polygon's orientation), so the new polygon is hpr_clip's up to a rotation of the
// array -- which changes nothing downstream.  `out` = number of outside vertices (0 < out < nv), f = the first
// of them (the one whose predecessor is inside).
__device__ __forceinline__ int hpr_clip_inplace(double2 *p, int ss, int nv, int out, int f, double A, double B, double C)
{
    const int ia = f ? f - 1 : nv - 1, ib = f;
    int ic = f + out - 1, id = f + out;
    ic -= ic >= nv ? nv : 0;
    id -= id >= nv ? nv : 0;
    const double2 va = p[(size_t)ia * ss], vb = p[(size_t)ib * ss], vc = p[(size_t)ic * ss], vd = p[(size_t)id * ss];
    const double sa = va.x * A + va.y * B - C, sb = vb.x * A + vb.y * B - C;
    const double sc = vc.x * A + vc.y * B - C, sd = vd.x * A + vd.y * B - C;
    double2 x1, x2;
    const bool h1 = sa != 0.0, h2 = sd != 0.0;          // (sb > 0 and sc > 0 always)
    {
        const double t = sa / (sa - sb);
        x1.x = va.x + t * (vb.x - va.x);
        x1.y = va.y + t * (vb.y - va.y);
    }
    {
        const double t = sc / (sc - sd);
        x2.x = vc.x + t * (vd.x - vc.x);
        x2.y = vc.y + t * (vd.y - vc.y);
    }
    const int e = (h1 ? 1 : 0) + (h2 ? 1 : 0);
    const double2 y0 = h1 ? x1 : x2;          // the crossings in order: y0 [, x2]
    const int m = nv - out + e;
    if (f + out <= nv) {
        // no wrap: [0, f) stays, the crossings, then the tail [f + out, nv) moved to f + e
        const int from = f + out, to = f + e, cnt = nv - from;
        if (to < from) {
            for (int k = 0; k < cnt; k++) p[(size_t)(to + k) * ss] = p[(size_t)(from + k) * ss];
        } else if (to > from) {
            for (int k = cnt - 1; k >= 0; k--) p[(size_t)(to + k) * ss] = p[(size_t)(from + k) * ss];
        }
        if (e > 0) p[(size_t)f * ss] = y0;
        if (e > 1) p[(size_t)(f + 1) * ss] = x2;
    } else {
        // the run wraps: the inside vertices [id, f) move to the front, the crossings follow
        const int cnt = f - id;
        if (id > 0)
            for (int k = 0; k < cnt; k++) p[(size_t)k * ss] = p[(size_t)(id + k) * ss];
        if (e > 0) p[(size_t)cnt * ss] = y0;
        if (e > 1) p[(size_t)(cnt + 1) * ss] = x2;
    }
    return m;
}

// What a polygon can reach: its largest squared vertex norm D^2 and its support max_v (v . d) in the eight
// directions d = (+-1, 0), (0, +-1), (+-1, +-1).  UPPER bounds suffice (they only feed conservative rejections),
// and a clip only shrinks the polygon, so these are refreshed now and then, not after every clip.
struct HprReach {
    double d2, xp, xn, yp, yn, pp, pn, np, nn;
};

__device__ __forceinline__ HprReach hpr_reach(const double2 *p, int ss, int nv)
{
    HprReach r;
    double d2 = 0.0, xp = -__builtin_inf(), xn = xp, yp = xp, yn = xp, pp = xp, pn = xp, np = xp, nn = xp;
    for (int k = 0; k < nv; k++) {
        const double2 v = p[(size_t)k * ss];
        const double r2 = v.x * v.x + v.y * v.y, s = v.x + v.y, t = v.x - v.y;
        d2 = r2 > d2 ? r2 : d2;
        xp = v.x > xp ? v.x : xp;   xn = -v.x > xn ? -v.x : xn;
        yp = v.y > yp ? v.y : yp;   yn = -v.y > yn ? -v.y : yn;
        pp = s > pp ? s : pp;       nn = -s > nn ? -s : nn;
        pn = t > pn ? t : pn;       np = -t > np ? -t : np;
    }
    r.d2 = d2;
    r.xp = xp; r.xn = xn; r.yp = yp; r.yn = yn; r.pp = pp; r.pn = pn; r.np = np; r.nn = nn;
    return r;
}

// True when the candidate's line a A + b B = C provably misses the polygon (then every vertex has
// a A + b B - C < 0 in floating point as well: the margins are 1e-9, the roundoff 1e-15).  Two bounds on
// max_v (a A + b B): Cauchy-Schwarz with the largest vertex norm, and -- for polygons that run out to the
// box in some directions (points on the silhouette) -- (A, B) split into its two neighbouring support
// directions: with a = |A| >= b = |B|, (A, B) = (a - b)(sx, 0) + b (sx, sy), so v.(A, B) <= (a-b) h(sx,0) + b h(sx,sy).
__device__ __forceinline__ bool hpr_far(const HprReach r, double A, double B, double C)
{
    if (C > 0.0 && r.d2 * (A * A + B * B) * 1.000000001 < C * C) return true;
    const double a = fabs(A), b = fabs(B);
    const double hx = A >= 0.0 ? r.xp : r.xn, hy = B >= 0.0 ? r.yp : r.yn;
    const double hd = A >= 0.0 ? (B >= 0.0 ? r.pp : r.pn) : (B >= 0.0 ? r.np : r.nn);
    const double t1 = a >= b ? (a - b) * hx : (b - a) * hy;
    const double t2 = (a >= b ? b : a) * hd;
    return t1 + t2 + 1e-9 * (fabs(t1) + fabs(t2) + fabs(C)) < C;
}

// Can any candidate of tile T cut the polygon?  Every candidate q = rho_q u_q of the tile has u_q within phi of
// the axis w and rho_q <= rho_max, so for a normal n:  n.q <= rho_max |n| cos(max(0, angle(n, w) - phi)).
// First for all n = u + d with |d| <= D at once (|n| <= L, angle(n, u) <= psi), then vertex by vertex.  The
// tile is skipped when the bound stays below |p'_i| (margins 1e-9 >> roundoff; squares instead of sqrt).
__device__ __forceinline__ bool hpr_tile_needed(const HprFrame &f, double cpsi, double spsi, const double2 *p, int ss, int nv,
                                                const HprTile &T)
{
    if (!(T.cos_phi > 0.0)) return true;
    const double uw = f.ux * T.wx + f.uy * T.wy + f.uz * T.wz;
    const double rr = f.rho * (1.0 - 1e-9) * T.inv_rho_max;
    {
        const double cc = T.cos_phi * cpsi - T.sin_phi * spsi;       // cos(phi + psi), psi = atan D
        const double sc = T.sin_phi * cpsi + T.cos_phi * spsi;       // sin(phi + psi)
        if (cc > 0.0 && uw < cc * (1.0 - 1e-9)) {                        // angle(u, w) > phi + psi
            const double rhs = rr * cpsi - 1e-9 - cc * uw;                 // cpsi = 1 / L, L = sqrt(1 + D^2) >= |n|
            const double s2 = sc * sc * ((1.0 - uw * uw) * (1.0 + 1e-9) + 1e-12);
            if (rhs > 0.0 && s2 < rhs * rhs) return false;
        }
    }
    const double e1w = f.e1x * T.wx + f.e1y * T.wy + f.e1z * T.wz;
    const double e2w = f.e2x * T.wx + f.e2y * T.wy + f.e2z * T.wz;
    for (int k = 0; k < nv; k++) {
        const double2 v = p[(size_t)k * ss];
        const double nn = 1.0 + v.x * v.x + v.y * v.y;
        const double dw = uw + v.x * e1w + v.y * e2w;
        if (dw > 0.0 && dw * dw >= T.cos2_phi * nn * (1.0 - 1e-9)) {
            if (!(nn < rr * rr)) return true;                            // n inside the cone: bound rho_max |n|
        } else {
            const double rhs = rr - 1e-9 * nn - T.cos_phi * dw;
            const double s2 = T.sin2_phi * ((nn - dw * dw) * (1.0 + 1e-9) + 1e-12 * nn);
            if (!(rhs > 0.0 && s2 < rhs * rhs)) return true;
        }
    }
    return false;
}

// tiles outward from the own one: step 0 = own, 1 = own + 1, 2 = own - 1, 3 = own + 2, ...
__device__ __forceinline__ int hpr_tile_of(int step, int own) { return (step & 1) ? own + (step + 1) / 2 : own - step / 2; }

// the tile a group of 128 consecutive listed points starts from: that of its middle point
__device__ __forceinline__ int hpr_base_tile(const int *hl, int nhard, int rank)
{
    int mid = (rank / kHprThreads) * kHprThreads + kHprThreads / 2;
    mid = mid < nhard ? mid : nhard - 1;
    return hl[mid] / kHprThreads;
}

// Blocks go to the 8 XCDs round-robin by linear id, each XCD with its own 4 MB L2.  1-D launches of ntiles blocks for each
// of c views, mapped so that the blocks of a view run on ONE XCD (c a multiple of 8; otherwise view-major order): they all
// read the view's flipped points and tile records, and with a view's blocks on eight XCDs every L2 held every view in flight
// (1 GB fetched from HBM per launch for 246 MB of input at 1024 x 10000).
__device__ __forceinline__ void hpr_block(int ntiles, int c, int &view, int &tile)
{
    const int lin = blockIdx.x;
    if ((c & 7) == 0) {
        const int xcd = lin & 7, k = lin >> 3;
        view = 8 * (k / ntiles) + xcd;
        tile = k % ntiles;
    } else {
        view = lin / ntiles;
        tile = lin % ntiles;
    }
}

// Parked points are stored in eight segments, one per XCD: the blocks of a view run on XCD view % 8 (hpr_block), one view
// after the other, so a segment holds its views' points grouped by view -- and the wave-per-point kernels send block b to
// segment b % 8 (the XCD it runs on), where consecutive waves then read ONE view's flipped points and tile records
// through that XCD's L2 (in one list in order of arrival every L2 saw eight to sixteen views at a time).
// base[x] = start of segment x (prefix sums of the views' listed points: upper bounds), status[kHprStSegFill + x] = its fill.
// The record lives in device memory, written by hpr_segs_kernel from the accept pass's per-view counts: the host never
// sees a count of this entry point (round 4 fetched six of them, a stream synchronisation each).
struct HprSegs {
    int base[9];
    int on;            // 0: one segment (views not a multiple of 8)
    int cap;           // slots the polygon store holds: a point whose slot lies beyond is listed (restarts from the box) instead of parked
};
static_assert(kHprStSegs * sizeof(int) + sizeof(HprSegs) <= kHprStatusWords * sizeof(int) && kHprStSegFill + 8 <= kHprStSegs &&
              kHprStBounds + 6 <= kHprStSegFill && kHprStUndecided < kHprStBounds,
              "the named words and the segment record share the 64-int header");
__device__ __forceinline__ int hpr_seg_of(const HprSegs &sg, int view) { return sg.on ? (view & 7) : 0; }
// item b of a pass over `8 x longest segment` (or the one segment): its slot, -1 past the segment's end
__device__ __forceinline__ int hpr_seg_slot(const HprSegs &sg, const int *status, int b)
{
    const int x = sg.on ? (b & 7) : 0, k = sg.on ? (b >> 3) : b;
    const int slot = sg.base[x] + k;
    return k < status[kHprStSegFill + x] && slot < sg.cap ? slot : -1;
}
// items of such a pass
__device__ __forceinline__ int hpr_seg_items(const HprSegs &sg, const int *status)
{
    int longest = 0;
    for (int x = 0; x < 8; x++) longest = max(longest, status[kHprStSegFill + x]);
    return sg.on ? 8 * longest : longest;
}

// tools/hpr_phases.py builds a private copy with -DGENPC_HPR_PROF: per block, shader-clock ticks of hpr_kernel's phases and
// the trip counts of its clip loop (slots 0 .. 8), the wave-per-point walk's figures (slots 9 .. 15), summed into g_hpr_prof
// (compiled out of the shipped library).  Without relocatable device code a file that counts holds an array of its own
// (HPR_PROF_ARRAY, with its reader); genpc_hpr_prof_read adds them.
#ifdef GENPC_HPR_PROF
#define HPR_PROF_ARRAY(reader) \
    static __device__ unsigned long long g_hpr_prof[16]; \
    bool reader(unsigned long long *out, int reset) \
    { \
        const unsigned long long z[16] = {0}; \
        return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_hpr_prof), sizeof z) == hipSuccess && \
               (!reset || hipMemcpyToSymbol(HIP_SYMBOL(g_hpr_prof), z, sizeof z) == hipSuccess); \
    }
bool hpr_first_prof_read(unsigned long long *out, int reset);
bool hpr_wave_prof_read(unsigned long long *out, int reset);
#define HPR_PROF_DECL unsigned long long prof_c[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define HPR_PROF_ADD(k, v) do { prof_c[k] += (unsigned long long)(v); } while (0)      // per lane, in registers
#define HPR_PROF_FLUSH() do { for (int k_ = 0; k_ < 10; k_++) { unsigned long long v_ = prof_c[k_]; if (k_ >= 4 && k_ != 8) { for (int o_ = 32; o_ > 0; o_ >>= 1) { const unsigned long long x_ = __shfl_xor(v_, o_, 64); v_ = k_ == 5 ? (x_ > v_ ? x_ : v_) : v_ + x_; } } \
        if ((threadIdx.x & 63) == 0) atomicAdd(&g_hpr_prof[k_], v_); } } while (0)
#define HPR_PROF_CLOCK() __builtin_readcyclecounter()
#else
#define HPR_PROF_ARRAY(reader)
#define HPR_PROF_DECL do {} while (0)
#define HPR_PROF_ADD(k, v) do {} while (0)
#define HPR_PROF_FLUSH() do {} while (0)
#define HPR_PROF_CLOCK() 0ull
#endif

// One call's arguments and the pieces hpr_run carved for it
struct HprCall {
    int c, n;
    const float *points;
    const double *eyes;
    double radius;
    unsigned char *visible;
    int *counts;
    int no_cull;
    // kWsHpr
    int *status, *list, *i0, *i1, *hardlist, *hardcnt, *und, *work;          // (und, alive: null unless views are pruned)
    double *fl;
    unsigned *k0, *k1;
    char *sort_tmp;
    size_t sort_bytes;
    HprTile *tiles;
    unsigned char *hard, *alive, *dup;
    int4 *surv;
    double2 *surv_poly, *gbuf;          // kWsHprParked (null: one-kernel form), kWsHprGlobalPolys
    unsigned *bounds() const { return (unsigned *)(status + kHprStBounds); }
    HprSegs *segs() const { return (HprSegs *)(status + kHprStSegs); }
};

// The passes, in the order hpr_run calls them; false: an error, recorded
bool hpr_sort_bytes(size_t pairs, hipStream_t stream, size_t &bytes);                      // hpr_order.hip: rocprim's scratch
bool hpr_launch_order(const HprPlan &plan, const HprCall &k, hipStream_t stream);          // hpr_order.hip: duplicates .. tile records
bool hpr_launch_accept(const HprPlan &plan, const HprCall &k, hipStream_t stream);         // hpr_accept.hip: accept, compact, segments
bool hpr_launch_first(const HprPlan &plan, const HprCall &k, hipStream_t stream);          // hpr_first.hip: first polygon pass, prune
bool hpr_launch_wave(const HprPlan &plan, const HprCall &k, hipStream_t stream);           // hpr_wave.hip: the wave-per-point passes, finish

}  // namespace genpc
