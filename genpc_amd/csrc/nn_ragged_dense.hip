// nn_ragged_dense.hip -- the ragged nearest neighbours by ALL PAIRS: every query of a pair against every target of it, in fp32,
// without a grid.  Its cost is n_j m_j whatever the clouds look like, which is what the ragged alignment loop wants: three of its
// four starts are turned by 90 / 180 / 270 degrees, their queries have no near target, and nn_ragged_kernel's lanes then walk
// hundreds of cells one dependent load after the other.  Opt-in (genpc_nn_ragged_tune); the answers are the
// grid search's, bit for bit.
//
// ONE launch, shaped by nn_ragged_dense_plan.h:
//   * an item is 64 queries of one pair in nn_ragged_kernel's numbering (ragged_table.h: ragged_items, ragged_pair_of); its
//     workgroup is four waves that hold the SAME 64 queries, one per lane;
//   * the pair's unsorted targets ([M,3] floats, as the caller packed them) pass through LDS in tiles of kNnDenseTile: the 256
//     threads fetch a tile's 3 kNnDenseTile floats with kNnDenseLoads coalesced dword loads each and store them as float4
//     (x, y, z, -); wave w scans targets [w kNnDenseShare, (w + 1) kNnDenseShare) of the tile, all lanes reading the same
//     address, so a target is one broadcast ds_read_b128;
//   * the NEXT tile's loads are issued before the current tile is scanned and land in registers meanwhile: an item has a handful
//     of tiles, and none of them starts cold;
//   * after the last tile waves 1 .. 3 hand their (distance, index) to wave 0 through the tile's LDS, and wave 0 writes.
// One query per lane, not two.  From MI355X's LDS table a ds_read_b128 costs 4 LDS cycles a wave-instruction whatever it
// broadcasts, and the compute unit's four SIMDs share one LDS: a target costs the unit 4 x 4 = 16 LDS cycles while each wave
// spends its inner loop's VALU instructions on it, 4 cycles each -- 40 cycles at the 10 counted below.  The scan is VALU-bound
// with the LDS 40 % busy; two queries a lane would halve the LDS share and double the registers of a loop that has no use for
// the slack.  (The compiler sees that w is never used and reads 12 of a target's 16 bytes: ds_read_b96, one instruction all
// the same.)
// The inner loop, sixteen targets unrolled, in the disassembly of this file (-O3, gfx950): per target one ds_read_b96 and
//   FMA    10 VALU: 3 v_sub_f32, v_mul_f32, 2 v_fmac_f32, v_cmp_lt_f32, 2 v_cndmask_b32 (distance, index), v_add_u32 (the
//                   candidate's index: 18 of them for 16 targets, the loop's counters among them)
//   strict 12 VALU: 3 v_sub_f32, 3 v_mul_f32, 2 v_add_f32, and the same four
// and 12 or 13 s_nop per sixteen targets between a compare and the select that reads its mask.  Both instantiations: 67 VGPRs,
// 53 SGPRs, no scratch, nothing spilled, 16400 bytes of LDS -- seven workgroups (28 waves) a compute unit.
// Measured: 64 pairs of about 900 x 4 500, 2.55e8 pair evaluations, take 83 us as 949 workgroups and 70 us as
// 4 557 -- ten instructions a pair at the chip's VALU rate are 65 us.
//
// The answer is nn_ragged_kernel's: the minimum of `distance bits << 32 | index inside the pair`.  A lane scans its targets in
// ascending order and replaces on a strict `<`, so it holds the lowest index among bit-equal distances of its share; the four
// waves' results are combined lexicographically.  The same minimum, because a squared distance of finite input is in [0, +inf]:
// never -0, never NaN.
// +inf IS A CANDIDATE LIKE ANY OTHER.  A lane starts from (+inf, kNone) and `<` never replaces that by a +inf distance, so kNone
// survives the combine exactly when no distance of the pair is below +inf, i.e. when all of them are +inf: the minimum key is
// then (+inf, 0), and that is what wave 0 writes for kNone (the pair has a target: a pair with queries and none is refused).
// Not finite (genpc_nm_distance_ragged's contract): a query with a non-finite coordinate gets (NaN, -1), and so does every
// query of a pair whose targets hold one.  The workgroup sees every target of its pair while staging; each thread keeps an OR
// over what it fetched, the OR over the workgroup is formed after the last tile and before the one place that writes results.
// Bounds: the tile loop runs ceil(m_j / kNnDenseTile) times, every fetch is below 3 m_j floats of the pair's slice, every LDS
// index below the tile; a lane writes only its own query's slot inside [qoff[j], qoff[j + 1]).  No spin, no atomics, no
// workspace.  A pair without queries costs at most one workgroup that leaves at once.
#include "nn.h"
#include "../../include/genpc_hip.h"

namespace genpc {

thread_local int t_nn_ragged_dense = 0;

constexpr int kNone = 0x7fffffff;          // no distance below +inf seen (above every index: at most 2^20 targets in a pair)

struct NnRaggedDenseArgs {
    RaggedTable t;
    const float *q;            // packed queries
    const float *tg;           // packed targets, as the caller has them
    float *out_d;              // packed like the queries
    int *out_i;
};
static_assert(sizeof(NnRaggedDenseArgs) <= 4096, "the pair table must fit the kernel arguments");

template <int FMA>
__global__ __launch_bounds__(kNnDenseThreads) void nn_ragged_dense_kernel(NnRaggedDenseArgs a)
{
    __shared__ float4 s_tile[kNnDenseTile];
    __shared__ int s_bad[kNnDenseWaves];
    const int item = blockIdx.x;
    const int pair = ragged_pair_of(a.t, item);
    const int q0 = a.t.qoff[pair], nq = a.t.qoff[pair + 1] - q0;
    const int first = (item - ((q0 >> 6) + pair)) * kNnDenseQueries;
    if (first >= nq) return;                                   // the pair's idle item (uniform: before any barrier)
    const int lane = threadIdx.x & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (uniform, and known to be)
    const int i = first + lane;
    const bool mine = i < nq;
    const size_t at = (size_t)q0 + (mine ? i : first);         // (a lane past the end scans for the item's first query and writes nothing)
    const float qx = a.q[at * 3 + 0], qy = a.q[at * 3 + 1], qz = a.q[at * 3 + 2];
    const float inf = __builtin_inff();
    const int t0 = a.t.toff[pair], m = a.t.toff[pair + 1] - t0;
    const float *__restrict__ T = a.tg + (size_t)t0 * 3;
    const long long floats = 3ll * m;
    const int tiles = (m + kNnDenseTile - 1) / kNnDenseTile;

    float nx[kNnDenseLoads];                                   // the next tile's floats threadIdx.x + 256 k
    auto fetch = [&](int tile) {
        const long long f0 = (long long)tile * (3 * kNnDenseTile) + threadIdx.x;
#pragma unroll
        for (int k = 0; k < kNnDenseLoads; k++) {
            const long long f = f0 + k * kNnDenseThreads;
            nx[k] = f < floats ? T[f] : 0.0f;
        }
    };
    int bad = 0;
    float bd = inf;
    int bi = kNone;
    fetch(0);
    for (int tile = 0; tile < tiles; tile++) {
        float *s = (float *)s_tile;
#pragma unroll
        for (int k = 0; k < kNnDenseLoads; k++) {
            const int f = threadIdx.x + k * kNnDenseThreads;   // float f of the tile: target f / 3, coordinate f % 3
            bad |= !(fabsf(nx[k]) < inf);
            s[(f / 3) * 4 + f % 3] = nx[k];
        }
        if (tile + 1 < tiles) fetch(tile + 1);                 // in flight across the scan below
        __syncthreads();
        const int base = tile * kNnDenseTile;
        const int cnt = m - base < kNnDenseTile ? m - base : kNnDenseTile;
        const int lo = wave * kNnDenseShare, hi = cnt < lo + kNnDenseShare ? cnt : lo + kNnDenseShare;
#pragma unroll 16
        for (int p = lo; p < hi; p++) {
            const float4 e = s_tile[p];
            const float dd = sqdist<FMA>(e.x - qx, e.y - qy, e.z - qz);
            const bool lt = dd < bd;
            bd = lt ? dd : bd;
            bi = lt ? base + p : bi;
        }
        __syncthreads();                                       // the tile is scanned: it may be overwritten
    }
    // the pair's flag, and the four waves' results for a query: both through LDS, before anything is written
    const int wave_bad = __ballot(bad != 0) != 0ull;
    if (lane == 0) s_bad[wave] = wave_bad;
    float *s_d = (float *)s_tile;
    int *s_i = (int *)s_tile + (kNnDenseWaves - 1) * kNnDenseQueries;
    if (wave > 0) {
        s_d[(wave - 1) * kNnDenseQueries + lane] = bd;
        s_i[(wave - 1) * kNnDenseQueries + lane] = bi;
    }
    __syncthreads();
    if (wave > 0 || !mine) return;
    int pair_bad = 0;
#pragma unroll
    for (int w = 0; w < kNnDenseWaves; w++) pair_bad |= s_bad[w];
#pragma unroll
    for (int w = 1; w < kNnDenseWaves; w++) {
        const float od = s_d[(w - 1) * kNnDenseQueries + lane];
        const int oi = s_i[(w - 1) * kNnDenseQueries + lane];
        const bool other = od < bd || (od == bd && oi < bi);
        bd = other ? od : bd;
        bi = other ? oi : bi;
    }
    if (bi == kNone) bi = 0;                                   // every distance of the pair is +inf: (+inf, 0), the head of this file
    if (pair_bad || !(fabsf(qx) < inf && fabsf(qy) < inf && fabsf(qz) < inf)) {
        bd = __builtin_nanf("");
        bi = -1;
    }
    a.out_d[at] = bd;
    a.out_i[at] = bi;
}

int nn_ragged_dense(const RaggedTable &t, const float *queries, const float *targets, float *d, int *i, hipStream_t st)
{
    const NnRaggedDensePlan plan = nn_ragged_dense_plan(t);
    if (plan.too_large) {
        set_error(plan.too_large);
        return 0;
    }
    if (plan.items <= 0) return 1;
    const int fma = arith_mode() != 0;
    NnRaggedDenseArgs a{};
    a.t = t; a.q = queries; a.tg = targets; a.out_d = d; a.out_i = i;
    if (fma) hipLaunchKernelGGL((nn_ragged_dense_kernel<1>), dim3((unsigned)plan.items), dim3(plan.threads), 0, st, a);
    else hipLaunchKernelGGL((nn_ragged_dense_kernel<0>), dim3((unsigned)plan.items), dim3(plan.threads), 0, st, a);
    return check(hipGetLastError(), "nn_ragged_dense_kernel launch") ? 1 : 0;
}

}  // namespace genpc

GENPC_API int genpc_nn_ragged_tune(int search)
{
    if (search != 0 && search != 1) {
        genpc::set_error("genpc_nn_ragged_tune: the search is 0 (grid) or 1 (dense)");
        return -1;
    }
    const int prev = genpc::t_nn_ragged_dense;
    genpc::t_nn_ragged_dense = search;
    return prev;
}

GENPC_API int genpc_nn_ragged_dense_plan(int c, const int *noff, const int *moff, int out[8])
{
    using namespace genpc;
    const char *fn = "genpc_nn_ragged_dense_plan";
    if (!out) return ragged_refuse(fn, "null output");
    for (int k = 0; k < 8; k++) out[k] = 0;
    out[1] = kNnDenseThreads; out[2] = kNnDenseQueries; out[3] = kNnDenseTile; out[4] = kNnDenseShare; out[5] = (int)kNnDenseLds;
    RaggedTable t;
    int max_targets = 0;
    const char *err = nullptr;
    const int rc = ragged_table_fill(c, noff, moff, t, &max_targets, &err);
    if (rc < 0) return ragged_refuse(fn, err);
    if (rc == 0) return 1;
    const NnRaggedDensePlan plan = nn_ragged_dense_plan(t);
    out[0] = (int)plan.items;                                  // (at most 2^22 + 384)
    out[1] = plan.threads; out[2] = plan.queries; out[3] = plan.tile; out[4] = plan.share; out[5] = plan.lds_bytes;
    out[6] = (int)(unsigned)(plan.evals & 0xffffffffll);       // the 64-bit count in two halves
    out[7] = (int)(plan.evals >> 32);
    return plan.too_large ? ragged_refuse(fn, plan.too_large) : 1;
}
