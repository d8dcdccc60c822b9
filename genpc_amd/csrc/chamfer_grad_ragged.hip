// chamfer_grad_ragged.hip -- genpc_chamfer_backward_ragged: the Chamfer backward over a ragged batch (the pairs of
// genpc_nm_distance_ragged, both directions), every gradient row summed in a STATED order and written once.  No
// floating-point atomic anywhere: the same bytes on every run, on every stream, wherever a pair stands in the call.
//
// The order is the CPU oracle's (oracle_chamfer_backward: direction 1 ascending, then direction 2 ascending):
//     gradxyz1[i] = +0  + v(i)                      then  - w(k) for k ascending with idx2[k] == i
//     gradxyz2[t] = +0  - v(i) for i ascending with idx1[i] == t      then  + w(t)
//     v(i) = (2 g1[i]) (A[i] - B[idx1[i]]),   w(k) = (2 g2[k]) (B[k] - A[idx2[k]])     per component, every operation rounded
// A term whose index is outside its pair's cloud (the forward's -1 for non-finite input) is absent in both places.
//
// Both directions share ONE numbering: rows 0 .. N-1 are xyz1's, rows N .. N+M-1 are xyz2's (N, M: the packed totals), and
// a term is known by the row that owns it.  Three steps, their number independent of c:
//   * chamfer_ragged_key_kernel: owner row q -> (key, q), key the row its term also lands on (N + moff[j] + idx1 for an
//     xyz1 row, noff[j] + idx2 for an xyz2 row), N + M for an absent term;
//   * rocprim's radix sort of the N + M pairs by key, over the bits N + M needs.  It is stable: inside a key the owners
//     ascend.  One sort serves both directions -- the keys of one are the owners of the other, so the ranges are disjoint;
//   * chamfer_ragged_grad_kernel: a lane per output row.  Its own term, a lower_bound of its row among the sorted keys, a
//     walk of that segment in order.  A row that thousands of terms land on (M_j = 1) is a long chain on one lane: the
//     order is the contract, and the other lanes do not wait for it beyond their own workgroup.
// The pair of a workgroup comes from the table in the kernel arguments as in nn_ragged.hip: 64 rows of ONE pair per
// workgroup, first the workgroups of xyz1's rows, then those of xyz2's.
#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"
#include "ragged_table.h"
#include "../../include/genpc_hip.h"

namespace genpc {

struct ChamferRaggedGradArgs {
    RaggedTable t;               // qoff: xyz1's rows per pair (noff), toff: xyz2's (moff)
    int items1;                  // workgroups of xyz1's rows; the rest serve xyz2's
    const float *xyz1, *xyz2, *gd1, *gd2;
    const int *idx1, *idx2;
    unsigned *keys, *vals;       // key kernel: written, row order; gradient kernel: read, sorted
    float *gx1, *gx2;
};
static_assert(sizeof(ChamferRaggedGradArgs) <= 4096, "the pair table must fit the kernel arguments");

// The row a lane serves.  side 0: row `at` of xyz1, whose index points into the pair's other[0 .. nother) of xyz2; side 1 the converse.
struct RaggedRow {
    int side, at, other0, nother;
    bool live;
};
__device__ __forceinline__ RaggedRow ragged_row(const ChamferRaggedGradArgs &a)
{
    RaggedRow r;
    r.side = (int)blockIdx.x >= a.items1;
    const int item = (int)blockIdx.x - (r.side ? a.items1 : 0);
    const int *mine = r.side ? a.t.toff : a.t.qoff, *theirs = r.side ? a.t.qoff : a.t.toff;
    const int pair = ragged_item_owner(mine, a.t.c, item, 6);          // (ragged_pair_of over either column of the table)
    const int r0 = mine[pair], nr = mine[pair + 1] - r0;
    const int i = (item - ((r0 >> 6) + pair)) * kRaggedLanes + (int)threadIdx.x;
    r.live = i < nr;
    r.at = r0 + i;
    r.other0 = theirs[pair];
    r.nother = theirs[pair + 1] - r.other0;
    return r;
}

__global__ __launch_bounds__(kRaggedLanes) void chamfer_ragged_key_kernel(ChamferRaggedGradArgs a)
{
    const RaggedRow r = ragged_row(a);
    if (!r.live) return;
    const unsigned n1 = (unsigned)a.t.qoff[a.t.c], total = n1 + (unsigned)a.t.toff[a.t.c];
    const int idx = (r.side ? a.idx2 : a.idx1)[r.at];
    const unsigned q = (r.side ? n1 : 0u) + (unsigned)r.at;
    const unsigned land = (r.side ? 0u : n1) + (unsigned)r.other0 + (unsigned)idx;
    a.keys[q] = (unsigned)idx < (unsigned)r.nother ? land : total;
    a.vals[q] = q;
}

__global__ __launch_bounds__(kRaggedLanes) void chamfer_ragged_grad_kernel(ChamferRaggedGradArgs a)
{
    const RaggedRow r = ragged_row(a);
    if (!r.live) return;
    const unsigned n1 = (unsigned)a.t.qoff[a.t.c], total = n1 + (unsigned)a.t.toff[a.t.c];
    const float *__restrict__ P = r.side ? a.xyz2 : a.xyz1;          // this row's cloud
    const float *__restrict__ O = r.side ? a.xyz1 : a.xyz2;          // the other cloud
    const float *__restrict__ GO = r.side ? a.gd1 : a.gd2;           // the other cloud's weights
    const size_t at = (size_t)r.at;
    const float px = P[at * 3 + 0], py = P[at * 3 + 1], pz = P[at * 3 + 2];

    // this row's own term: first on an xyz1 row, last on an xyz2 row
    const int idx = (r.side ? a.idx2 : a.idx1)[at];
    const bool own = (unsigned)idx < (unsigned)r.nother;
    float ox = 0.0f, oy = 0.0f, oz = 0.0f;
    if (own) {
        const size_t j = (size_t)r.other0 + (size_t)idx;
        const float g = __fmul_rn((r.side ? a.gd2 : a.gd1)[at], 2.0f);
        ox = __fmul_rn(g, px - O[j * 3 + 0]);
        oy = __fmul_rn(g, py - O[j * 3 + 1]);
        oz = __fmul_rn(g, pz - O[j * 3 + 2]);
    }
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    if (own && !r.side) { sx = __fadd_rn(sx, ox); sy = __fadd_rn(sy, oy); sz = __fadd_rn(sz, oz); }

    // the terms that land here, in the order of their owners
    const unsigned row = (r.side ? n1 : 0u) + (unsigned)r.at, back = r.side ? 0u : n1;
    const unsigned *__restrict__ K = a.keys, *__restrict__ V = a.vals;
    unsigned lo = 0, hi = total;
    while (lo < hi) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        if (K[mid] < row) lo = mid + 1; else hi = mid;
    }
    for (unsigned p = lo; p < total && K[p] == row; p++) {
        const size_t k = (size_t)(V[p] - back);                      // a row of the other cloud whose index names this one
        const float g = __fmul_rn(GO[k], 2.0f);
        const float tx = __fmul_rn(g, O[k * 3 + 0] - px), ty = __fmul_rn(g, O[k * 3 + 1] - py), tz = __fmul_rn(g, O[k * 3 + 2] - pz);
        sx = __fadd_rn(sx, -tx); sy = __fadd_rn(sy, -ty); sz = __fadd_rn(sz, -tz);
    }
    if (own && r.side) { sx = __fadd_rn(sx, ox); sy = __fadd_rn(sy, oy); sz = __fadd_rn(sz, oz); }
    float *__restrict__ out = r.side ? a.gx2 : a.gx1;
    out[at * 3 + 0] = sx; out[at * 3 + 1] = sy; out[at * 3 + 2] = sz;
}

static int chamfer_backward_ragged(ChamferRaggedGradArgs &a, hipStream_t st)
{
    const int c = a.t.c;
    const size_t total = (size_t)a.t.qoff[c] + (size_t)a.t.toff[c];        // <= 2^29
    unsigned bits = 1;
    while ((total >> bits) != 0) bits++;                                   // the keys are 0 .. total
    unsigned *k0, *v0, *k1, *v1;
    char *tmp;
    size_t sort_bytes = 0;
    if (!check(rocprim::radix_sort_pairs(nullptr, sort_bytes, (const unsigned *)nullptr, (unsigned *)nullptr, (const unsigned *)nullptr,
                                         (unsigned *)nullptr, total, 0u, bits, st), "chamfer_backward_ragged sort sizing"))
        return 0;
    WsLayout L;
    L.add(k0, total);
    L.add(v0, total);
    L.add(k1, total);
    L.add(v1, total);
    L.add(tmp, sort_bytes);
    if (!ws_alloc(L, kWsChamferRaggedGrad, st)) return 0;
    a.items1 = (int)ragged_items(a.t.qoff[c], c);
    const unsigned grid = (unsigned)(a.items1 + ragged_items(a.t.toff[c], c));
    a.keys = k0; a.vals = v0;
    hipLaunchKernelGGL(chamfer_ragged_key_kernel, dim3(grid), dim3(kRaggedLanes), 0, st, a);
    if (!check(hipGetLastError(), "chamfer_ragged_key_kernel launch")) return 0;
    if (!check(rocprim::radix_sort_pairs(tmp, sort_bytes, (const unsigned *)k0, k1, (const unsigned *)v0, v1, total, 0u, bits, st),
               "chamfer_backward_ragged radix sort"))
        return 0;
    a.keys = k1; a.vals = v1;
    hipLaunchKernelGGL(chamfer_ragged_grad_kernel, dim3(grid), dim3(kRaggedLanes), 0, st, a);
    return check(hipGetLastError(), "chamfer_ragged_grad_kernel launch") ? 1 : 0;
}

}  // namespace genpc

GENPC_API int genpc_chamfer_backward_ragged(int c, const int *noff, const float *xyz1, const int *moff, const float *xyz2,
                                            const float *graddist1, const int *idx1, const float *graddist2, const int *idx2,
                                            float *gradxyz1, float *gradxyz2, void *stream)
{
    using namespace genpc;
    ChamferRaggedGradArgs a{};
    RaggedTable converse;              // checked, not used: it is a.t with the columns exchanged
    int max_other = 0;
    const char *err = nullptr;
    const int rc1 = ragged_table_fill(c, noff, moff, a.t, &max_other, &err);
    const int rc2 = rc1 < 0 ? rc1 : ragged_table_fill(c, moff, noff, converse, &max_other, &err);
    if (rc1 < 0 || rc2 < 0) {
        char msg[160];
        snprintf(msg, sizeof msg, "genpc_chamfer_backward_ragged: %s (%s)", err, rc1 < 0 ? "xyz1 against xyz2" : "xyz2 against xyz1");
        set_error(msg);
        return -1;
    }
    // (a pair empty on one side only was refused in one of the two roles: with rows on either side, both tables are filled)
    if (rc1 == 0 || rc2 == 0) return 1;
    if (!xyz1 || !xyz2 || !graddist1 || !idx1 || !graddist2 || !idx2 || !gradxyz1 || !gradxyz2) {
        set_error("genpc_chamfer_backward_ragged: null pointer");
        return -1;
    }
    a.xyz1 = xyz1; a.xyz2 = xyz2; a.gd1 = graddist1; a.gd2 = graddist2; a.idx1 = idx1; a.idx2 = idx2;
    a.gx1 = gradxyz1; a.gx2 = gradxyz2;
    return chamfer_backward_ragged(a, (hipStream_t)stream);
}
