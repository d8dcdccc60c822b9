// fps.hip -- farthest point sampling for gfx950 (the metric of
// main.py:21-24 subsamples both clouds to 16384 points before CD/EMD, reg_xyz.py:215
// samples 20000 fused points).  The reference calls fpsample.fps_sampling, a
// third-party CPU extension with a RANDOM start index (not reproducible, unpinned);
// this is the deterministic counterpart used by the fixtures: start index 0, fp32
// squared distances, first arg-max.  Bit-exact with oracle_fps.
//
// FPS is k strictly sequential steps of (update N running minima, arg-max): what a step
// costs is the LATENCY of its dependency chain, not bandwidth (a step touches no memory but
// the hand-off).  Round 3 layout, built around that chain (round 2: 2.8 us per step):
//   * a cloud is owned by W <= 64 workgroups of 192 worker threads; every thread keeps R <= 24 points and their
//     running minima in REGISTERS for the whole run -- 192 to 4608 points per workgroup, one wave per
//     SIMD (round 2: 16 points on each of 16 waves of one CU, 1.2 us of VALU issue per step);
//   * a thread carries the coordinates of its best point along, the wave's best is found with DPP row
//     rotations + v_readlane (no LDS round trips), the workgroup's best with one LDS exchange;
//   * the hand-off carries the candidates' COORDINATES: four 8-byte write-through stores per candidate,
//     {dist, gen | idx} {x, gen} {y, gen} {z, gen}, each self-tagged with the exchange's generation (the
//     8-byte granule written by one store is the unit whose atomicity the hardware documents; round 2 published
//     the index alone and every workgroup then fetched the pivot from memory: one more dependent miss);
//   * one wave per workgroup polls the cloud's W slots (a lane per slot), picks the global winner
//     and hands the pivot to its workgroup through LDS.  Slots are double-buffered by step parity: no
//     reset, no fences, no grid barrier.
// Several clouds -- of DIFFERENT sizes and sample counts -- run side by side in one launch (grid.y):
// the two subsamplings of the metric and the fused cloud's can share one pass (genpc_fps_multi).
// This file is the multi-workgroup sampler alone: the kernel, the one table of its instantiations and fps_multi_run, which carries
// out the launches fps_plan.h planned.  Which of the library's three samplers a cloud takes (this one: clouds of 24577 to 262144
// points, and smaller ones under genpc_fps_tune(256)), a cloud's workgroups and points per thread, and which clouds share a launch
// are fps_plan.h's decisions; fps_call.hip holds the entry points, fps_verify.hip the check every finished sequence gets.
// All workgroups of a launch must be co-resident: launches are sized from what the device holds of the instantiation they take
// (fps_device) and admitted through the budget the one-launch auction shares.  The polls are bounded all the same:
// a hand-off that times out aborts the cloud's run (every workgroup leaves its step loop), raises the error
// word and writes -1 to out[0]; genpc_amd/fps.py raises on it.
#include "fps.h"
#include "../../include/genpc_hip.h"

namespace genpc {

constexpr int kFWaves = kFThreads / kWave;
static_assert(kFMaxW * kFMaxR * kFThreads >= kFpsMultiMaxN, "what the plan sends to fps_kernel fits its registers");

// Wave-wide integer max / min, uniform result, in seven instructions: four row rotations (each one v_max_i32 with a
// DPP operand -- written in assembly: the compiler emits v_mov_b32 + v_mov_b32_dpp + v_max_i32 per step) leave every
// row's result in all of its lanes, row_bcast:15 / row_bcast:31 fold the rows into lane 63, one v_readlane fetches it.
// (s_nop 1: a VGPR written by a VALU instruction needs two wait states before a DPP read.)
#define GENPC_WAVE_REDUCE_I32(OP)                                                                         \
    int r;                                                                                                \
    asm volatile("s_nop 1\n\t"                                                                            \
                 OP " %0, %1, %1 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"                                 \
                 "s_nop 1\n\t"                                                                            \
                 OP " %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"                                 \
                 "s_nop 1\n\t"                                                                            \
                 OP " %0, %0, %0 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"                                 \
                 "s_nop 1\n\t"                                                                            \
                 OP " %0, %0, %0 row_ror:1 row_mask:0xf bank_mask:0xf\n\t"                                 \
                 "s_nop 1\n\t"                                                                            \
                 OP " %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"                              \
                 "s_nop 1\n\t"                                                                            \
                 OP " %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"                              \
                 "s_nop 1"                                                                                \
                 : "=&v"(r)                                                                               \
                 : "v"(v));                                                                               \
    return __builtin_amdgcn_readlane(r, 63);

__device__ __forceinline__ int wave_min_i32(int v) { GENPC_WAVE_REDUCE_I32("v_min_i32_dpp") }
__device__ __forceinline__ int wave_max_i32_dpp(int v) { GENPC_WAVE_REDUCE_I32("v_max_i32_dpp") }

__device__ __forceinline__ float lane_f32(float v, int lane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// 8-byte write-through stores and L1-bypassing 16-byte loads (sc0 sc1: what agent-scope relaxed atomics lower to
// for 8 bytes).  A 16-byte load may see its two granules at different times: each carries its own tag.
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void store_sc_b64(void *p, uint2 v)
{
    const u32x2 w = {v.x, v.y};
    asm volatile("global_store_dwordx2 %0, %1, off sc0 sc1" ::"v"(p), "v"(w) : "memory");
}

constexpr int kFT = 4;          // candidates a workgroup publishes per exchange
constexpr int kFBatch = 64;     // most samples drawn from one exchange
constexpr int kFBlock = kFThreads + kWave;     // three waves own the points, a fourth coordinates: each has a SIMD to itself (a fifth
                                               // wave shared its SIMD with a worker, and the replay -- a chain of dependent
                                               // cross-lane steps -- got every other issue slot: 1200 cycles per pick)

struct FpsCand {          // 32 bytes = four self-tagged 8-byte granules, each written by ONE write-through store (the
    uint4 a;              //   documented single-copy-atomic unit): {dist bits, gen << 20 | idx} {x bits, gen}
    uint4 b;              //   {y bits, gen} {z bits, gen}.  Read back as two 16-byte loads; every half carries its tag.
};
struct FpsSlot {          // one 128-byte line per (job, parity, workgroup)
    FpsCand c[kFT];
};

// the eight loads of one slot in flight together, one wait
__device__ __forceinline__ void load_slot(const FpsSlot *p, u32x4 (&a)[kFT], u32x4 (&b)[kFT])
{
    static_assert(kFT == 4 && sizeof(FpsCand) == 32, "offsets below");
    asm volatile("global_load_dwordx4 %0, %8, off sc0 sc1\n\t"
                 "global_load_dwordx4 %4, %8, off offset:16 sc0 sc1\n\t"
                 "global_load_dwordx4 %1, %8, off offset:32 sc0 sc1\n\t"
                 "global_load_dwordx4 %5, %8, off offset:48 sc0 sc1\n\t"
                 "global_load_dwordx4 %2, %8, off offset:64 sc0 sc1\n\t"
                 "global_load_dwordx4 %6, %8, off offset:80 sc0 sc1\n\t"
                 "global_load_dwordx4 %3, %8, off offset:96 sc0 sc1\n\t"
                 "global_load_dwordx4 %7, %8, off offset:112 sc0 sc1\n\t"
                 "s_waitcnt vmcnt(0)"
                 : "=&v"(a[0]), "=&v"(a[1]), "=&v"(a[2]), "=&v"(a[3]), "=&v"(b[0]), "=&v"(b[1]), "=&v"(b[2]), "=&v"(b[3])
                 : "v"(p)
                 : "memory");
}

// One exchange among a cloud's workgroups yields SEVERAL samples, exactly:
//   every workgroup lists its kFT best points in the order (distance desc, index asc) with their coordinates;
//   every workgroup reads all lists and replays the sequential algorithm on the listed points alone -- pick the
//   best, lower the listed distances by the pick, pick again ...  A pick is the true next sample as long as its
//   key is not below tau = the best of the workgroups' LAST listed keys (as listed): every unlisted point of a
//   workgroup ranks below that workgroup's last listed point, and distances only fall.  The first pick of an
//   exchange always qualifies, so a round never stalls; with points dealt to workgroups round-robin the top of
//   the global order is spread over many lists and a round draws tens of samples (measured: 30 at 172000
//   points, 13 at 16384, 8.5 at 8192).
// Inside a workgroup: waves 0..2 own the points (registers); wave 3, the coordinator, owns none.  It merges the
// waves' lists, publishes, polls, replays -- and hands every pick to the workers through LDS (s_piv + a progress
// word) the moment it is made, so the workers lower their running minima WHILE the replay goes on (the replay is a
// chain of dependent cross-lane steps, ~400 cycles per pick, and would otherwise leave three SIMDs idle).  One
// barrier per round: workers' lists ready -> coordinator.
constexpr unsigned kProgDone = 0x8000u, kProgFinal = 0x4000u, kProgAbort = 0x2000u, kProgCount = 0x0fffu;

// The progress word and the pivots it announces are both LDS, written by ONE wave and read by the others: the LDS unit
// serves a wave's requests in issue order, so "pivot, then word" on the writer and "word, then pivot" on the readers
// need no hardware fence -- only the compiler must keep the order (a release / acquire pair at workgroup scope also
// waits for the wave's outstanding GLOBAL stores: ~500 cycles per pick next to the 16-byte publishes).
__device__ __forceinline__ void prog_store(unsigned *p, unsigned v)
{
    // The pivots are 16-byte LDS writes, the word a 4-byte one: the wave's earlier LDS writes are PERFORMED before the word is
    // issued (lgkmcnt counts LDS operations only: ~60 cycles, no global store is waited for).  Belt and braces -- the
    // failure that prompted it (round 4: a sampling next to the f16 nearest-neighbour filter on another stream drew a sample
    // too early, silently) turned out to sit on the readers' side: see the workers' pivot reads.
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    asm volatile("" ::: "memory");
}
__device__ __forceinline__ unsigned prog_load(unsigned *p)
{
    asm volatile("" ::: "memory");
    const unsigned v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    asm volatile("" ::: "memory");
    return v;
}

// The lane with the wave's best key.  Distances are >= 0 or one of the negative sentinels (-1 padding, -2 dead),
// never NaN: the signed-integer order of their bit patterns ranks every live value above every sentinel and agrees
// with the float order among live values, so the maximum is ONE integer reduction (fmaxf would canonicalise every
// operand first).  Ties (equal distances) take the index reduction.
__device__ __forceinline__ int wave_argbest(float v, int idx, float &m)
{
    const int vb = __float_as_int(v);
    const int mb = wave_max_i32_dpp(vb);
    m = __int_as_float(mb);
    const unsigned long long mask = __ballot(vb == mb);
    if (__popcll(mask) == 1) return __ffsll((long long)mask) - 1;
    const int cand = vb == mb ? idx : 0x7fffffff;
    const int best = wave_min_i32(cand);
    return __ffsll((long long)__ballot(cand == best)) - 1;
}

// The body of the sampling.
template <int FMA, int R>
static __device__ __forceinline__ void fps_body(const FpsJobs &jobs, FpsSlot *slots, int *__restrict__ err)
{
    __shared__ float s_c[kFWaves][kFT][5];     // per worker wave: dist, idx (bits), x, y, z of its kFT best
    __shared__ float s_piv[kFBatch][4];        // the round's pivots: x, y, z, idx (bits)
    // ... and the same pivots as three SELF-TAGGED 8-byte granules {x, tag} {y, tag} {z, tag}, tag = round * 64 + slot + 1: what
    // the workers read.  A worker takes a pivot only when all three tags of ITS OWN copy are the expected one and re-reads
    // otherwise, so a lane that is handed the previous occupant of the slot (round 4: lanes 48-63 next to another stream's f16
    // MFMAs, mechanism unknown; round 5: a wrong sample again with the pivot taken through scalar registers, next to the
    // one-launch auction) cannot lower its minima by it -- the hand-off no longer depends on what caused that.
    __shared__ uint2 s_pivt[kFBatch][3];
    __shared__ float s_pd[kFBatch];            // the round's picks: their running minimum when drawn
    __shared__ unsigned s_prog;                // round << 16 | flags | pivots of that round published so far
    const int job = blockIdx.y, wg = blockIdx.x, t = threadIdx.x;
    const int W = jobs.W[job];
    if (wg >= W) return;
    const int n = jobs.n[job], k = jobs.k[job];
    const int lane = t & (kWave - 1), wave = t >> 6;
    const float *__restrict__ X = jobs.xyz[job];
    if (t == 0) s_prog = 0xffff0000u;          // no round carries this tag
    __syncthreads();

    if (wave < kFWaves) {
        // ------------------------------------------------------------------ workers
        // points are dealt round-robin: point i belongs to workgroup i % W (a file's scan order would otherwise
        // give every workgroup one compact patch, and a patch's best points fall together)
        float px[R], py[R], pz[R], d[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const long long i = ((long long)r * kFThreads + t) * W + wg;
            const bool ok = i < n;
            const size_t ii = ok ? (size_t)i : (size_t)(n - 1);
            px[r] = X[ii * 3 + 0];
            py[r] = X[ii * 3 + 1];
            pz[r] = X[ii * 3 + 2];
            d[r] = ok ? __builtin_inff() : -1.0f;          // -1: never selected, never updated upward
        }
        for (unsigned round = 0;; round++) {
            // ---- lower the running minima by the round's pivots as the coordinator hands them over
            unsigned applied = 0, pr;
            for (;;) {
                pr = prog_load(&s_prog);
                if ((pr >> 16) != (round & 0xffffu)) { __builtin_amdgcn_s_sleep(1); continue; }
                const unsigned avail = pr & kProgCount;
                auto apply_pivot = [&]() {
                    // The pivot travels through SCALAR registers (first lane's copy).  As plain per-lane reads of the one LDS
                    // address (ds_read_b96 into VGPRs, consumed by packed fp32 ops right behind the wait) the lanes 48-63 of a
                    // worker wave were seen to use the PREVIOUS pivot now and then while another stream's kernel issued
                    // v_mfma_f32_32x32x16_f16 on the same SIMD -- one stale running minimum, one sample drawn a step early, the
                    // rest of the sequence shifted by one, no error (tools/stress_concurrent.py: every run with the f16
                    // filter or tools/burn.hip's bare MFMA loop next to it, never alone, never next to fp32 MFMA / LDS / VALU
                    // loads; all extra samples were points held by lanes 48-63).  The mechanism is not established (an isolated
                    // probe of broadcast reads + packed adds under the same load, tools/lds_probe.hip, shows nothing); with the
                    // value in SGPRs nine of nine stress runs are clean.  tests/test_gpu_concurrency.py keeps watch.
                    const unsigned want = (round & 0x3ffffffu) * 64u + applied + 1u;
                    uint2 g0, g1, g2;
                    int tries = 0;
                    bool good;
                    do {
                        asm volatile("" ::: "memory");      // (re-read from LDS on every trip)
                        const unsigned long long *gp = (const unsigned long long *)&s_pivt[applied][0];
                        const unsigned long long w0 = __hip_atomic_load(gp + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        const unsigned long long w1 = __hip_atomic_load(gp + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        const unsigned long long w2 = __hip_atomic_load(gp + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        g0 = make_uint2((unsigned)w0, (unsigned)(w0 >> 32));
                        g1 = make_uint2((unsigned)w1, (unsigned)(w1 >> 32));
                        g2 = make_uint2((unsigned)w2, (unsigned)(w2 >> 32));
                        good = g0.y == want && g1.y == want && g2.y == want;
                    } while (!__all(good) && ++tries < 4096);
                    // ... and the VALUE every lane uses is lane 0's copy, through scalar registers (round 5: with six scans in flight
                    // 8 % of the samplings failed the device-side check, and every wrong sample -- 44 of 44 -- was a point held in
                    // REGISTER 0 by lanes 48-63 of a worker wave, its running minimum not lowered by one pivot: the first arithmetic
                    // behind the wait used the previous occupant of the value register in the last sixteen lanes although the tag
                    // registers of the same loads, compared later, were current)
                    const float cx = __uint_as_float(__builtin_amdgcn_readfirstlane(g0.x));
                    const float cy = __uint_as_float(__builtin_amdgcn_readfirstlane(g1.x));
                    const float cz = __uint_as_float(__builtin_amdgcn_readfirstlane(g2.x));
                    // What the wrong samples were (round 5; six scans in flight): written plainly, the compiler pairs registers
                    // r, r + 1 into PACKED fp32 instructions whose subtracts take ONE half of a source pair for both lanes
                    // (v_pk_add_f32 ... op_sel_hi:[1,0] / op_sel:[0,1]), and beside other streams' kernels 8 % of the samplings then
                    // failed the device-side check -- every first wrong sample, 55 of 55, a point held in the LOW lane of a pair
                    // (register 0) by lanes 48-63 of a worker wave whose running minimum had missed one pivot.  It reproduces in a
                    // plain HIP program: tools/opsel_probe.hip, v_pk_add_f32 ... op_sel:[0,1] on known data beside tools/burn.hip's
                    // MFMA kernel on another stream -- 2.5e9 wrong results in 5 s, all in lanes 48-63, all the low lane's, as if the
                    // selected half were 0 (op_sel_hi / plain: none; tools/PACKED_FP32_OPSEL.md).  Hence one register at a time (the
                    // opaque statements keep the compiler from pairing), and the whole library is built without packed fp32
                    // instructions (genpc_amd/build.py).
#pragma unroll
                    for (int r = 0; r < R; r++) {
                        float dx = px[r] - cx, dy = py[r] - cy, dz = pz[r] - cz;
                        asm volatile("" : "+v"(dx), "+v"(dy), "+v"(dz));
                        float dd = sqdist<FMA>(dx, dy, dz);
                        asm volatile("" : "+v"(dd));
                        d[r] = d[r] < dd ? d[r] : dd;       // padding slots stay at -1
                    }
                };
                for (; applied < avail; applied++) apply_pivot();
                if (pr & kProgDone) break;
            }
            if (pr & (kProgFinal | kProgAbort)) break;
            // ---- the wave's kFT best, best first
            unsigned taken = 0;
#pragma unroll
            for (int c = 0; c < kFT; c++) {
                float bv = -2.0f, bx = 0.0f, by = 0.0f, bz = 0.0f;
                int br = 0;
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const bool gt = !((taken >> r) & 1u) && d[r] > bv;    // ascending index within a thread: first max
                    bv = gt ? d[r] : bv;
                    br = gt ? r : br;
                    bx = gt ? px[r] : bx;
                    by = gt ? py[r] : by;
                    bz = gt ? pz[r] : bz;
                }
                const int bi = bv > -2.0f ? (int)((((long long)br * kFThreads + t) * W + wg)) : 0x7fffffff;
                float mx;
                const int src = wave_argbest(bv, bi, mx);
                // (cross-lane reads in wave-uniform code: inside a lane-0 branch the compiler may copy a value with
                // an exec-masked move, and v_readlane would then fetch another lane's stale register)
                const float wi = __int_as_float(__builtin_amdgcn_readlane(bi, src));
                const float w0 = lane_f32(bx, src), w1 = lane_f32(by, src), w2 = lane_f32(bz, src);
                if (lane == 0) {
                    s_c[wave][c][0] = mx;
                    s_c[wave][c][1] = wi;
                    s_c[wave][c][2] = w0;
                    s_c[wave][c][3] = w1;
                    s_c[wave][c][4] = w2;
                }
                if (lane == src) taken |= 1u << br;
            }
            __syncthreads();                   // lists ready -> coordinator
        }
        return;
    }

    // ---------------------------------------------------------------------- coordinator (the last wave)
    int *__restrict__ out = jobs.out[job];
    float *__restrict__ pdist = jobs.pdist[job];
    FpsSlot *S = slots + jobs.slot0[job];
    int s = 1;                                 // samples drawn so far
    if (lane == 0) {
        s_piv[0][0] = X[0]; s_piv[0][1] = X[1]; s_piv[0][2] = X[2];
        s_piv[0][3] = __int_as_float(0);
        s_pivt[0][0] = make_uint2(__float_as_uint(X[0]), 1u);      // round 0, slot 0
        s_pivt[0][1] = make_uint2(__float_as_uint(X[1]), 1u);
        s_pivt[0][2] = make_uint2(__float_as_uint(X[2]), 1u);
        if (wg == 0) { out[0] = 0; pdist[0] = __builtin_inff(); }
        prog_store(&s_prog, (0u << 16) | kProgDone | (k <= 1 ? kProgFinal : 0u) | 1u);
    }
    bool timed_out = false;
    unsigned round = 0;
    while (s < k) {
        __syncthreads();                       // the workers' lists of this round
        round++;
        // ---- the workgroup's kFT best of the waves' lists (lanes 0..15 hold one entry each)
        float ev = -2.0f, ex = 0.0f, ey = 0.0f, ez = 0.0f;
        int ei = 0x7fffffff;
        if (lane < kFWaves * kFT) {
            const float *e = &s_c[lane / kFT][lane % kFT][0];
            ev = e[0]; ei = __float_as_int(e[1]); ex = e[2]; ey = e[3]; ez = e[4];
        }
        float cd[kFT], cxs[kFT], cys[kFT], czs[kFT];
        int ci[kFT];
#pragma unroll
        for (int c = 0; c < kFT; c++) {
            float mx;
            const int src = wave_argbest(ev, ei, mx);
            cd[c] = mx;
            ci[c] = __builtin_amdgcn_readlane(ei, src);
            cxs[c] = lane_f32(ex, src); cys[c] = lane_f32(ey, src); czs[c] = lane_f32(ez, src);
            if (lane == src) ev = -2.0f;
        }
        if (W > 1) {
            const unsigned gen = (round % 4095u) + 1u;
            FpsSlot *slot = S + (size_t)(round & 1u) * W;
            if (lane < kFT) {
                // lane c publishes candidate c; an entry without a live point (dist < 0) carries index 0xFFFFF
                float pd = cd[0], pxx = cxs[0], pyy = cys[0], pzz = czs[0];
                int pi = ci[0];
#pragma unroll
                for (int c = 1; c < kFT; c++)
                    if (lane == c) { pd = cd[c]; pi = ci[c]; pxx = cxs[c]; pyy = cys[c]; pzz = czs[c]; }
                const unsigned pidx = pd >= 0.0f ? (unsigned)pi : 0xFFFFFu;
                uint2 *g = (uint2 *)&slot[wg].c[lane];
                store_sc_b64(g + 0, make_uint2(__float_as_uint(pd), (gen << 20) | pidx));
                store_sc_b64(g + 1, make_uint2(__float_as_uint(pxx), gen));
                store_sc_b64(g + 2, make_uint2(__float_as_uint(pyy), gen));
                store_sc_b64(g + 3, make_uint2(__float_as_uint(pzz), gen));
            }
            // every lane < W reads workgroup `lane`'s list, bounded
            u32x4 a[kFT];
            u32x4 b[kFT];
#pragma unroll
            for (int c = 0; c < kFT; c++) { a[c] = (u32x4){0, 0, 0, 0}; b[c] = (u32x4){0, 0, 0, 0}; }
            int spins = 0;
            for (;;) {
                bool ready = true;
                if (lane < W) {
                    load_slot(&slot[lane], a, b);
#pragma unroll
                    for (int c = 0; c < kFT; c++) ready = ready && (a[c].y >> 20) == gen && a[c].w == gen && b[c].y == gen && b[c].w == gen;
                }
                if (__all(ready)) break;
                if (++spins > (1 << 21)) {
                    if (lane == 0) __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    timed_out = true;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            if (timed_out) break;
#pragma unroll
            for (int c = 0; c < kFT; c++) {
                const bool live = lane < W && (a[c].y & 0xFFFFFu) != 0xFFFFFu;
                cd[c] = live ? __uint_as_float(a[c].x) : -2.0f;
                ci[c] = live ? (int)(a[c].y & 0xFFFFFu) : 0x7fffffff;
                cxs[c] = __uint_as_float(a[c].z);
                cys[c] = __uint_as_float(b[c].x);
                czs[c] = __uint_as_float(b[c].z);
            }
        } else if (lane != 0) {
#pragma unroll
            for (int c = 0; c < kFT; c++) { cd[c] = -2.0f; ci[c] = 0x7fffffff; }
        }
        // ---- replay the sequential algorithm on the listed points (a lane per workgroup's list)
        // tau: the best of the lists' last entries, as listed (a list that is not full bounds nothing)
        float td;
        const int ti = __builtin_amdgcn_readlane(ci[kFT - 1], wave_argbest(cd[kFT - 1], ci[kFT - 1], td));
        int mm = 0;
        for (;;) {
            float ld = cd[0], lx = cxs[0], ly = cys[0], lz = czs[0];
            int li = ci[0];
#pragma unroll
            for (int c = 1; c < kFT; c++) {
                const bool better = (cd[c] > ld) | ((cd[c] == ld) & (ci[c] < li));
                ld = better ? cd[c] : ld;
                li = better ? ci[c] : li;
                lx = better ? cxs[c] : lx;
                ly = better ? cys[c] : ly;
                lz = better ? czs[c] : lz;
            }
            float md;
            const int src = wave_argbest(ld, li, md);
            const int mi = __builtin_amdgcn_readlane(li, src);
            const float qx = lane_f32(lx, src), qy = lane_f32(ly, src), qz = lane_f32(lz, src);
            if ((mm > 0) & !((md > td) | ((md == td) & (mi <= ti)))) break;
            if (lane == 0) {
                s_piv[mm][0] = qx; s_piv[mm][1] = qy; s_piv[mm][2] = qz;
                s_piv[mm][3] = __int_as_float(mi);
                s_pd[mm] = md;
                const unsigned tag = (round & 0x3ffffffu) * 64u + (unsigned)mm + 1u;
                s_pivt[mm][0] = make_uint2(__float_as_uint(qx), tag);
                s_pivt[mm][1] = make_uint2(__float_as_uint(qy), tag);
                s_pivt[mm][2] = make_uint2(__float_as_uint(qz), tag);
            }
            mm++;
            if (s + mm >= k || mm == kFBatch) break;
            if (lane == 0) prog_store(&s_prog, (round << 16) | (unsigned)mm);       // the workers may take it
#pragma unroll
            for (int c = 0; c < kFT; c++) {
                // (one candidate at a time, like the workers' update: no packed fp32 instructions)
                float dx = cxs[c] - qx, dy = cys[c] - qy, dz = czs[c] - qz;
                asm volatile("" : "+v"(dx), "+v"(dy), "+v"(dz));
                float dd = sqdist<FMA>(dx, dy, dz);
                asm volatile("" : "+v"(dd));
                cd[c] = cd[c] < dd ? cd[c] : dd;        // dead entries stay at -2
            }
        }
        if (lane == 0) prog_store(&s_prog, (round << 16) | kProgDone | (s + mm >= k ? kProgFinal : 0u) | (unsigned)mm);
        // the samples of the round, after the workers have been released (no global store inside the pick loop)
        if (wg == 0 && lane < mm) { out[s + lane] = __float_as_int(s_piv[lane][3]); pdist[s + lane] = s_pd[lane]; }
        s += mm;
    }
    if (timed_out && lane == 0) prog_store(&s_prog, (round << 16) | kProgDone | kProgAbort);
    // a hand-off that timed out (workgroups of a cloud not co-resident) poisons the result visibly: index 0 is
    // always 0 in a good run.  The other workgroups' coordinators time out once on the missing list and leave too.
    if (wg == 0 && lane == 0) {
        if (timed_out || __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) out[0] = -1;
        err[1 + jobs.stat0 + job] = (int)round;          // exchanges this cloud took (genpc_fps_stats)
    }
}

template <int FMA, int R>
__global__ __launch_bounds__(kFBlock) void fps_kernel(FpsJobs jobs, FpsSlot *slots, int *__restrict__ err)
{
    fps_body<FMA, R>(jobs, slots, err);
}

// THE dispatch over the register classes (fps_plan.h: kFpsClassPoints, fps_class): the instantiation of class cls, for the launch
// and for the occupancy query alike -- a launch is sized from the occupancy of the very kernel it takes.
typedef void (*FpsKernel)(FpsJobs, FpsSlot *, int *);
template <int FMA>
static FpsKernel fps_kernel_of(int cls)
{
    static_assert(kFpsClasses == 6, "an entry per class");
    static const FpsKernel table[kFpsClasses] = {fps_kernel<FMA, kFpsClassPoints[0]>, fps_kernel<FMA, kFpsClassPoints[1]>,
                                                 fps_kernel<FMA, kFpsClassPoints[2]>, fps_kernel<FMA, kFpsClassPoints[3]>,
                                                 fps_kernel<FMA, kFpsClassPoints[4]>, fps_kernel<FMA, kFpsClassPoints[5]>};
    return table[cls];
}

// Workgroups of an instantiation one CU holds at a time, as the runtime reports it (registers: fps_kernel<*, 16> is 152
// VGPRs = 3 per CU, <*, 24> 224 VGPRs = 2; the smaller ones 4+), asked once per arithmetic mode.  The hand-off between a cloud's
// workgroups needs ALL of the launch resident together, so launches are sized from this, not from a constant (a budget
// of four per CU admitted grids of the two large instantiations that an idle full chip just holds and a busy or partitioned one
// does not).
bool fps_device(bool fma, FpsDevice &dev)
{
    static int cache[2][kFpsClasses] = {{0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};
    int id = 0;
    if (!check(hipGetDevice(&id), "hipGetDevice")) return false;
    if (!check(hipDeviceGetAttribute(&dev.cus, hipDeviceAttributeMultiprocessorCount, id), "hipDeviceGetAttribute")) return false;
    if (dev.cus < 1) dev.cus = 1;
    int *nb = cache[fma ? 1 : 0];
    for (int cls = 0; cls < kFpsClasses; cls++) {
        if (nb[cls] < 1) {
            const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb[cls], fma ? fps_kernel_of<1>(cls) : fps_kernel_of<0>(cls), kFBlock, 0);
            if (e != hipSuccess || nb[cls] < 1) nb[cls] = 1;
        }
        dev.blocks_per_cu[cls] = nb[cls];
    }
    return true;
}

static_assert(sizeof(FpsSlot) == kFpsSlotBytes, "what fps_call reserves per slot");

// Clouds `sel[0 .. )` (indices into the call's arrays) through the multi-workgroup kernel, in the launches the plan made of them
// (shape and slot0 per selected cloud): admission, launch, and the check of the launch's clouds in line.
int fps_multi_run(const FpsCall &c, const int *sel, const FpsShape *shape, int nl, const FpsLaunch *launches, const int *slot0, void *slots)
{
    for (int l = 0; l < nl; l++) {
        const FpsLaunch &la = launches[l];
        FpsJobs jobs = {};
        jobs.stat0 = sel[la.first] < 32 ? sel[la.first] : 32;
        for (int q = 0; q < la.count; q++) {
            fps_fill_job(jobs, q, c, sel[la.first + q]);
            jobs.W[q] = shape[la.first + q].W;
            jobs.slot0[q] = slot0[la.first + q];
        }
        const FpsKernel kernel = c.fma ? fps_kernel_of<1>(fps_class(la.rmax)) : fps_kernel_of<0>(fps_class(la.rmax));
        const bool admitted = persist_reserve(la.units, emd_auction_capacity(), c.st);
        hipLaunchKernelGGL(kernel, dim3(la.wmax, la.count), dim3(kFBlock), 0, c.st, jobs, (FpsSlot *)slots, c.err);
        if (admitted) persist_commit(la.units, c.st);
        fps_verify(c, jobs, la.count, false);
    }
    return check(hipGetLastError(), "fps_kernel launch") ? 1 : 0;
}

}  // namespace genpc
