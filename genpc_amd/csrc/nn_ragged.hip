// nn_ragged.hip -- genpc_nm_distance over a ragged batch: c independent (queries, targets) pairs of any sizes, packed, one call.
//
// Two launches whatever c is (ragged_table.h: the pair table rides in the kernel arguments, nothing is copied or read back):
//   * grid.hip's ragged build sorts every pair's targets into an x-fastest grid of its own (grid.h), sized for that cloud;
//   * nn_ragged_kernel: a workgroup is one wave and serves up to 64 queries of ONE pair -- it finds the pair by a binary search
//     of the table (uniform: scalar loads), so the grid header, the cell table and the sorted cloud are the same for all its
//     lanes.  A lane owns a query, walks its pair's grid with grid.h's cell_grid_shell_walk and keeps one 64-bit key, distance
//     bits << 32 | index inside the pair's target cloud (nn_grid.hip's, knn_query.hip's): the minimum key is the nearest target,
//     the lowest index among bit-equal distances.  The distance is sqdist<FMA> of common.h in the call's arithmetic mode: on
//     finite clouds the bits of genpc_nm_distance(1, n_j, .., m_j, ..).  A distance that overflows to +inf is a candidate like
//     any other (all of them +inf: index 0, as there).
//   * not finite: a query with a non-finite coordinate, and every query of a pair whose targets hold one (CellGridHdr.bad,
//     decided by the build), gets (NaN, -1); the other pairs of the call do not notice.
// One path for every size: a tiny or degenerate cloud is a one-cell grid.  The queries are not reordered by cell: a wave's
// 64 queries are 64 neighbours in the caller's order, and the clouds this is for (hundreds to thousands of targets, 16 bytes
// each sorted) stay in the caches whatever the order (DESIGN_NOTEBOOK.md, "Ragged nearest neighbours").
#include "nn.h"
#include "../../include/genpc_hip.h"

namespace genpc {

constexpr unsigned long long kNRNone = 0x7f800000ffffffffull;    // (+inf, -1): above every candidate, +inf included

struct NnRaggedArgs {
    RaggedTable t;
    const float *q;            // packed queries
    const float4 *sorted;      // packed targets, every pair's slice in its own cell order: (x, y, z, index inside the pair)
    const int *start;          // pair j's cell table at toff[j] + 65 j
    const CellGridHdr *hdr;    // [c]
    float *out_d;              // packed like the queries
    int *out_i;
};
static_assert(sizeof(NnRaggedArgs) <= 4096, "the pair table must fit the kernel arguments");

template <int FMA>
__global__ __launch_bounds__(kRaggedLanes) void nn_ragged_kernel(NnRaggedArgs a)
{
    const int item = blockIdx.x;
    const int pair = ragged_pair_of(a.t, item);
    const int q0 = a.t.qoff[pair], nq = a.t.qoff[pair + 1] - q0;
    const int i = (item - ((q0 >> 6) + pair)) * kRaggedLanes + threadIdx.x;
    if (i >= nq) return;
    const size_t at = (size_t)q0 + i;
    const float qx = a.q[at * 3 + 0], qy = a.q[at * 3 + 1], qz = a.q[at * 3 + 2];
    const CellGridHdr H = a.hdr[pair];
    const float inf = __builtin_inff();
    if (H.bad || !(fabsf(qx) < inf && fabsf(qy) < inf && fabsf(qz) < inf)) {
        a.out_d[at] = __builtin_nanf("");
        a.out_i[at] = -1;
        return;
    }
    const int t0 = a.t.toff[pair];
    const float4 *__restrict__ S = a.sorted + t0;
    const int *__restrict__ ST = a.start + ((size_t)t0 + (size_t)kRaggedStartPad * pair);

    unsigned long long best = kNRNone;
    auto kth = [&]() { return __uint_as_float((unsigned)(best >> 32)); };      // +inf until a finite distance is held
    auto run = [&](int p0, int p1) {
        for (int p = p0; p < p1; p++) {
            const float4 e = S[p];
            const float dd = sqdist<FMA>(e.x - qx, e.y - qy, e.z - qz);
            const unsigned long long key = ((unsigned long long)__float_as_uint(dd) << 32) | (unsigned)__float_as_int(e.w);
            best = key < best ? key : best;          // (finite input: dd is in [0, +inf], so the keys order as the distances do)
        }
    };
    cell_grid_shell_walk(H, ST, qx, qy, qz, kth, run);
    a.out_d[at] = __uint_as_float((unsigned)(best >> 32));
    a.out_i[at] = (int)(unsigned)best;
}

// The call in its two halves (nn.h): the grids of the targets, and the search of them.
void nn_ragged_grids_layout(WsLayout &L, NnRaggedGrids &g, const RaggedTable &t)
{
    const int c = t.c;
    L.add(g.hdr, c);
    L.add(g.start, (size_t)ragged_start_len(t.toff[c], c));
    L.add(g.sorted, (size_t)t.toff[c]);
}

int nn_ragged_build(const RaggedTable &t, int max_targets, const float *xyz2, const NnRaggedGrids &g, hipStream_t st)
{
    return launch_cell_grid_build_ragged(t, max_targets, xyz2, (CellGridHdr *)g.hdr, (int *)g.start, (float4 *)g.sorted, st);
}

int nn_ragged_search(const RaggedTable &t, const float *xyz, const NnRaggedGrids &g, float *result, int *result_i, hipStream_t st)
{
    const int fma = arith_mode() != 0;
    NnRaggedArgs a{};
    a.t = t; a.q = xyz; a.out_d = result; a.out_i = result_i;
    a.hdr = g.hdr; a.start = g.start; a.sorted = g.sorted;
    const unsigned grid = (unsigned)ragged_items(t.qoff[t.c], t.c);
    if (fma) hipLaunchKernelGGL((nn_ragged_kernel<1>), dim3(grid), dim3(kRaggedLanes), 0, st, a);
    else hipLaunchKernelGGL((nn_ragged_kernel<0>), dim3(grid), dim3(kRaggedLanes), 0, st, a);
    return check(hipGetLastError(), "nn_ragged_kernel launch") ? 1 : 0;
}

static int nn_ragged(const RaggedTable &t, int max_targets, const float *xyz, const float *xyz2, float *result, int *result_i, hipStream_t st)
{
    NnRaggedGrids g{};
    WsLayout L;
    nn_ragged_grids_layout(L, g, t);
    if (!ws_alloc(L, kWsNnRagged, st)) return 0;
    if (!nn_ragged_build(t, max_targets, xyz2, g, st)) return 0;
    return nn_ragged_search(t, xyz, g, result, result_i, st);
}

}  // namespace genpc

GENPC_API int genpc_nm_distance_ragged(int c, const int *noff, const float *xyz, const int *moff, const float *xyz2, float *result,
                                       int *result_i, void *stream)
{
    using namespace genpc;
    RaggedTable t;
    int max_targets = 0;
    const char *err = nullptr;
    const int rc = ragged_table_fill(c, noff, moff, t, &max_targets, &err);
    if (rc < 0) return ragged_refuse("genpc_nm_distance_ragged", err);
    if (rc == 0) return 1;
    if (!xyz || !xyz2 || !result || !result_i) {
        set_error("genpc_nm_distance_ragged: null pointer");
        return -1;
    }
    if (t_nn_ragged_dense) {          // the thread's choice (genpc_nn_ragged_tune): all pairs, one launch, no workspace (nn_ragged_dense.hip)
        if (const char *why = nn_ragged_dense_plan(t).too_large) return ragged_refuse("genpc_nm_distance_ragged", why);
        return nn_ragged_dense(t, xyz, xyz2, result, result_i, (hipStream_t)stream);
    }
    return nn_ragged(t, max_targets, xyz, xyz2, result, result_i, (hipStream_t)stream);
}
