// scale_search_ragged.hip -- genpc_scale_search_scores over a ragged batch: c (source, target) pairs of any sizes, each with its
// own candidate scales, scored in one call (the fine xyz search of reg_xyz.py:60-96 for S scans at once).
//
// genpc_scale_search_scores (icp.hip) writes k scaled copies of the source and k copies of the target, runs every pair of points of
// every candidate through nn_forward and sums two arrays of distances.  Here nothing proportional to the candidates is written:
//   * all candidates of a pair share ONE target cloud: grid.hip's ragged build sorts every pair's target into an x-fastest grid
//     of its own (grid.h), once per call;
//   * scale_search_ragged_kernel: one workgroup of kIBlock threads per candidate.  It finds its pair by a binary search of the
//     table in the kernel arguments (uniform: scalar loads), scales the pair's source by its three scales and sorts the scaled
//     cloud into a grid in LDS (scale_search_ragged_plan.h; grid.h's box, sizing, scan and cell function); then thread t takes
//     the source points t, t + kIBlock, ... -- each walks the pair's target grid in global memory -- and the target points
//     t, t + kIBlock, ... -- each walks the grid in LDS --, both with grid.h's cell_grid_shell_walk, and adds the square roots of
//     the nearest distances in cd_score.h's order, which is cd_score_kernel's.
// The nearest distance is a minimum over sqdist<FMA> values and does not depend on how it is found; the sums are taken in one
// stated order: on finite input a candidate's score is the bits of genpc_scale_search_scores on its pair alone, in both
// arithmetic modes.  No floating-point atomic anywhere: the same bits on every run.  (The order of the points inside a cell is
// whatever the LDS atomics give; it reaches no result.)
// Not finite: a pair whose target holds a non-finite coordinate (CellGridHdr.bad) gets NaN for all its scores, a candidate whose
// scaled source holds one gets NaN; nobody else notices.
// A pair whose source does not fit the LDS is scored inside the same call by genpc_scale_search_scores on its slices.
#include "grid.h"
#include "cd_score.h"
#include "scale_search_ragged_plan.h"
#include "ragged_cand.h"
#include "../../include/genpc_hip.h"

namespace genpc {

static_assert(kSsBlock == kIBlock && kSsWaves * kWave == kIBlock, "scale_search_ragged_plan.h counts cd_score.h's workgroup");
static_assert(kSsRaggedMaxPairs == GENPC_SCALE_SEARCH_RAGGED_MAX_PAIRS, "the header exports the bound");
static_assert(kSsRaggedMaxPairs <= kRaggedMaxPairs, "the target grids are built through a RaggedTable");
static_assert(kSsFixed % 16 == 0, "the sorted cloud is read 16 bytes at a time");
static_assert(kSsRaggedMaxPairs == kRaggedCandMaxPairs && kSsRaggedMaxPoints == kRaggedCandMaxPoints &&
              kSsRaggedMaxCandidates == kRaggedCandMaxCandidates, "ragged_cand.h checks and carries the table");

struct ScaleSearchRaggedArgs {
    RaggedCandTable t;                         // (first: the layout of the kernel arguments)
    const float *source, *target;              // packed
    const float *scales;                       // [K,3]
    const CellGridHdr *hdr;                    // [c] the targets' grids: headers,
    const int *start;                          //   pair j's cell table at toff[j] + 65 j,
    const float4 *sorted;                      //   its targets in cell order at toff[j]
    float *scores;                             // [K]
    float w;
};
static_assert(sizeof(ScaleSearchRaggedArgs) <= 4096, "the pair table must fit the kernel arguments");

// the nearest squared distance from (qx, qy, qz) to the cloud sorted into the grid (H, ST, S): nn_ragged_kernel's walk, the distance
// alone.  A run is read kSsRunWidth points at a time (as icp_scan_cell reads four: that many loads in flight instead of one per
// trip of a loop whose every trip waits for its own load; the last group repeats the run's last point, which a minimum does not see).
constexpr int kSsRunWidth = 8;
template <int FMA>
__device__ __forceinline__ float scale_search_nearest(const CellGridHdr &H, const int *__restrict__ ST, const float4 *__restrict__ S,
                                                      float qx, float qy, float qz)
{
    float best = __builtin_inff();
    auto kth = [&]() { return best; };
    auto run = [&](int p0, int p1) {
        for (int p = p0; p < p1; p += kSsRunWidth) {
            float4 e[kSsRunWidth];
            float dd[kSsRunWidth];
#pragma unroll
            for (int u = 0; u < kSsRunWidth; u++) e[u] = S[min(p + u, p1 - 1)];
#pragma unroll
            for (int u = 0; u < kSsRunWidth; u++) dd[u] = sqdist<FMA>(e[u].x - qx, e[u].y - qy, e[u].z - qz);
#pragma unroll
            for (int u = 0; u < kSsRunWidth; u++) best = dd[u] < best ? dd[u] : best;          // (finite input: dd is in [0, +inf])
        }
    };
    cell_grid_shell_walk(H, ST, qx, qy, qz, kth, run);
    return best;
}

template <int FMA>
__global__ __launch_bounds__(kIBlock) void scale_search_ragged_kernel(ScaleSearchRaggedArgs a)
{
    extern __shared__ __align__(16) unsigned char ss_lds[];
    const int cand = blockIdx.x, tid = threadIdx.x;
    const int pair = ragged_cand_pair_of(a.t, cand), s0 = a.t.soff[pair], t0 = a.t.toff[pair];
    const int ns = a.t.soff[pair + 1] - s0, nt = a.t.toff[pair + 1] - t0;
    const ScaleSearchPlan plan = scale_search_plan(ns);
    if (!plan.one_workgroup) return;                   // (uniform: the whole workgroup leaves; the single call scores this pair)
    const CellGridHdr HT = a.hdr[pair];
    if (HT.bad) {                                      // (uniform)
        if (tid == 0) a.scores[cand] = __builtin_nanf("");
        return;
    }
    float *s_red = (float *)ss_lds;                                  // [6 waves] the box
    int *s_w = (int *)(s_red + 6 * kSsWaves);                        // [2 waves] the scan
    double *red = (double *)(s_w + 2 * kSsWaves);                    // [2 waves] the score
    float4 *P = (float4 *)(ss_lds + kSsFixed);                       // [ns] the scaled source in cell order: x, y, z, index
    int *T = (int *)(P + ns);                                        // [cells + 1] first position of every cell, then ns
    const float *__restrict__ src = a.source + (size_t)s0 * 3;
    const float *__restrict__ tgt = a.target + (size_t)t0 * 3;
    const double sc[3] = {(double)a.scales[(size_t)cand * 3 + 0], (double)a.scales[(size_t)cand * 3 + 1], (double)a.scales[(size_t)cand * 3 + 2]};
    // point j of the candidate's cloud: replicate_scale_kernel's statement
    auto scaled = [&](int j, float &x, float &y, float &z) {
        x = (float)((double)src[(size_t)j * 3 + 0] * sc[0]);
        y = (float)((double)src[(size_t)j * 3 + 1] * sc[1]);
        z = (float)((double)src[(size_t)j * 3 + 2] * sc[2]);
    };

    // ---- the grid of the scaled cloud, in LDS: the box of the SCALED points (a negative or tiny scale needs no special case)
    float mn[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float mx[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    int bad = 0;
    for (int j = tid; j < ns; j += kIBlock) {
        float p[3];
        scaled(j, p[0], p[1], p[2]);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (fabsf(p[k]) < __builtin_inff()) {
                mn[k] = fminf(mn[k], p[k]);
                mx[k] = fmaxf(mx[k], p[k]);
            } else {
                bad = 1;
            }
        }
    }
    grid_block_box<kIBlock>(mn, mx, s_red);
    if (__syncthreads_or(bad)) {                       // a non-finite scale, or a product that overflows
        if (tid == 0) a.scores[cand] = __builtin_nanf("");
        return;
    }
    CellGridHdr H;
    grid_size<16, false>(mn, mx, scale_search_cells_target(ns, plan.cells), plan.cells, H);
    H.cells = H.g[0] * H.g[1] * H.g[2];
    H.bad = 0;
    const int cells = H.cells;
    int *cnt = T + 1;                                  // counts, then starts, then ends of the cells: T[c + 1] = end of c = start of c + 1
    for (int q = tid; q < cells; q += kIBlock) cnt[q] = 0;
    if (tid == 0) T[0] = 0;
    __syncthreads();
    auto cell_of = [&](float x, float y, float z) {
        return (grid_cell1(z, H.lo[2], H.inv, H.g[2]) * H.g[1] + grid_cell1(y, H.lo[1], H.inv, H.g[1])) * H.g[0] + grid_cell1(x, H.lo[0], H.inv, H.g[0]);
    };
    for (int j = tid; j < ns; j += kIBlock) {
        float x, y, z;
        scaled(j, x, y, z);
        atomicAdd(&cnt[cell_of(x, y, z)], 1);
    }
    __syncthreads();
    grid_scan_counts<kIBlock>(cnt, cells, 0, s_w);
    for (int j = tid; j < ns; j += kIBlock) {
        float x, y, z;
        scaled(j, x, y, z);
        const int pos = atomicAdd(&cnt[cell_of(x, y, z)], 1);
        P[pos] = make_float4(x, y, z, __int_as_float(j));
    }
    __syncthreads();

    // ---- the two sums, each thread's points in cd_score.h's order
    const float4 *__restrict__ ST_sorted = a.sorted + t0;
    const int *__restrict__ ST = a.start + ((size_t)t0 + (size_t)kRaggedStartPad * pair);
    const double s1 = cd_score_thread_sum(ns, [&](int j) {
        float x, y, z;
        scaled(j, x, y, z);
        return scale_search_nearest<FMA>(HT, ST, ST_sorted, x, y, z);
    });
    const double s2 = cd_score_thread_sum(nt, [&](int j) {
        return scale_search_nearest<FMA>(H, T, P, tgt[(size_t)j * 3 + 0], tgt[(size_t)j * 3 + 1], tgt[(size_t)j * 3 + 2]);
    });
    cd_score_reduce(s1, s2, ns, nt, a.w, red, a.scores + cand);
}

}  // namespace genpc

GENPC_API int genpc_scale_search_scores_ragged(int c, const int *soff, const int *toff, const int *koff, const float *source,
                                               const float *target, const float *scales, float cd_inv_weight, float *scores, void *stream)
{
    using namespace genpc;
    const char *fn = "genpc_scale_search_scores_ragged";
    // every refusal is decided here, before anything touches a device: ragged_cand.h's about the table, then the payload
    const char *what = nullptr;
    char buf[96];
    const int work = ragged_cand_check(c, soff, toff, koff, &what, buf);
    if (work <= 0) return work < 0 ? ragged_refuse(fn, what) : 1;
    const int k = koff[c];
    if (!source || !target || !scales || !scores) return ragged_refuse(fn, "null pointer");
    hipStream_t st = (hipStream_t)stream;

    // the pairs of the one launch: those with candidates whose source gets the one-workgroup plan.  Their targets' grids are
    // built through a RaggedTable whose query side counts one for each of them and nothing for the others: those are not built.
    RaggedTable t;
    t.c = c;
    t.qoff[0] = 0;
    int fused = 0, loop = 0, max_targets = 0;
    size_t lds = 0;
    for (int j = 0; j < c; j++) {
        const int kj = koff[j + 1] - koff[j], nt = toff[j + 1] - toff[j];
        const ScaleSearchPlan p = scale_search_plan(soff[j + 1] - soff[j]);
        const bool in = kj > 0 && p.one_workgroup;
        t.qoff[j + 1] = t.qoff[j] + (in ? 1 : 0);
        t.toff[j] = toff[j];
        if (in) {
            fused++;
            if ((size_t)p.lds_bytes > lds) lds = (size_t)p.lds_bytes;
            if (nt > max_targets) max_targets = nt;
        } else if (kj > 0) {
            loop++;
        }
    }
    for (int j = c; j <= kRaggedMaxPairs; j++) t.toff[j] = toff[c];
    for (int j = c + 1; j <= kRaggedMaxPairs; j++) t.qoff[j] = t.qoff[c];
    if (fused) {
        ScaleSearchRaggedArgs a{};
        WsLayout L;
        L.add(a.hdr, c);
        L.add(a.start, (size_t)ragged_start_len(toff[c], c));
        L.add(a.sorted, (size_t)toff[c]);
        if (!ws_alloc(L, kWsScaleSearchRagged, st)) return 0;
        const int fma = arith_mode() != 0 ? 1 : 0;
        static size_t set_bytes[2] = {0, 0};
        if (lds > set_bytes[fma]) {
            const hipError_t e = fma ? hipFuncSetAttribute((const void *)scale_search_ragged_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)
                                     : hipFuncSetAttribute((const void *)scale_search_ragged_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (!check(e, "hipFuncSetAttribute(scale_search_ragged_kernel)")) return 0;
            set_bytes[fma] = lds;
        }
        if (!launch_cell_grid_build_ragged(t, max_targets, target, (CellGridHdr *)a.hdr, (int *)a.start, (float4 *)a.sorted, st)) return 0;
        ragged_cand_fill(a.t, c, soff, toff, koff);
        a.source = source; a.target = target; a.scales = scales; a.scores = scores;
        a.w = cd_inv_weight;
        // one workgroup per candidate of the call; those of a pair of the single call leave at once
        if (fma) hipLaunchKernelGGL((scale_search_ragged_kernel<1>), dim3(k), dim3(kIBlock), lds, st, a);
        else hipLaunchKernelGGL((scale_search_ragged_kernel<0>), dim3(k), dim3(kIBlock), lds, st, a);
        if (!check(hipGetLastError(), "scale_search_ragged_kernel launch")) return 0;
    }
    if (loop) {
        for (int j = 0; j < c; j++) {
            const int kj = koff[j + 1] - koff[j], ns = soff[j + 1] - soff[j];
            if (kj == 0 || scale_search_plan(ns).one_workgroup) continue;
            const int rc = genpc_scale_search_scores(kj, ns, source + (size_t)soff[j] * 3, toff[j + 1] - toff[j], target + (size_t)toff[j] * 3,
                                                     scales + (size_t)koff[j] * 3, cd_inv_weight, scores + koff[j], stream);
            if (rc != 1) return rc < 0 ? 0 : rc;
        }
    }
    return 1;
}

GENPC_API int genpc_scale_search_ragged_plan(int c, const int *soff, int out[3])
{
    using namespace genpc;
    const char *fn = "genpc_scale_search_ragged_plan";
    if (!out) return ragged_refuse(fn, "null pointer");
    out[0] = out[1] = out[2] = 0;
    const char *what = nullptr;
    const int some = ragged_cand_count(c, &what);
    if (some <= 0) return some < 0 ? ragged_refuse(fn, what) : 1;
    if (!soff) return ragged_refuse(fn, "null offset table");
    if ((what = ragged_offsets_fault(c, soff))) return ragged_refuse(fn, what);
    const ScaleSearchRaggedPlan p = scale_search_ragged_plan(c, soff);
    out[0] = p.fused_pairs;
    out[1] = p.loop_pairs;
    out[2] = p.lds_bytes;
    return 1;
}
