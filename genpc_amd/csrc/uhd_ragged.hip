// uhd_ragged.hip -- genpc_uhd over a ragged batch: c independent (queries, targets) pairs of any sizes, packed, one call.
//
// Pair j's answer is genpc_uhd's for that pair alone: d2 = max_i min_j s_ij with uhd.h's uhd_s (fp64 on the widened fp32
// coordinates, nothing fused), i* the lowest query that attains it, j* the lowest target of the pair with s == d2 for query i*.
// Four launches whatever c is; the pair table (ragged_table.h) rides in the kernel arguments, nothing is copied or read back:
//   * uhd_ragged_init_kernel: one fp64 word per query of the call, set to +inf.
//   * uhd_ragged_pairs_kernel: uhd_pairs_kernel's loop.  A workgroup owns up to 1024 queries of ONE pair (blockIdx.x is a work
//     item of ragged_items.h's numbering with shift 10; the pair comes from a binary search of the table, uniform: scalar loads)
//     and the kUhdTile targets number blockIdx.y of that pair; a workgroup past its pair's queries or targets leaves at once.
//     So one pair of 10000 x 20000 is spread over 10 x 40 workgroups as genpc_uhd spreads it.  Each lane folds its four minima
//     into the queries' words with a 64-bit INTEGER atomic minimum on the bit pattern: every s is +0, positive or +inf (fmin
//     has dropped the NaNs and the minimum starts at +inf), so the unsigned order of the bits is the numeric order, and an
//     integer minimum is exact and does not depend on the order of arrival -- the word ends as the same bits on every run.
//     No floating-point atomic anywhere.
//   * uhd_ragged_query_kernel: the same work items; a lane reads its four queries' minima, the workgroup keeps the greatest
//     (uhd_beats: the lowest query among equals) as one record per item.  An idle item writes a record that loses to all.
//   * uhd_ragged_finish_kernel: one workgroup per pair reduces its items' records the same way to (d2, i*), then re-evaluates
//     query i* against all the pair's targets -- the same operations give the same bits -- and takes the lowest j with s == d2
//     (the minimum word does not say which tile it came from, so there is no tile to confine the search to: ceil(M_j / 256)
//     steps a thread, 79 for 20000 targets).
// Scratch: 8 bytes a query and 16 bytes a work item.  A NaN pair of points is skipped by fmin; include/genpc_hip.h says what
// non-finite input returns.  Everything is enqueued on the caller's stream.
#include "uhd.h"
#include "ragged_items.h"
#include "../../include/genpc_hip.h"

namespace genpc {

constexpr int kUhdRaggedShift = 10;               // a work item: kUhdBlock * kUhdQ = 1024 queries of one pair
static_assert((1 << kUhdRaggedShift) == kUhdBlock * kUhdQ, "a work item is what a workgroup of uhd_pairs_kernel owns");
constexpr unsigned long long kUhdInfBits = 0x7ff0000000000000ull;

struct UhdRaggedArgs {
    RaggedTable t;
    const float *q;                // packed queries
    const float *tg;               // packed targets
    unsigned long long *qmin;      // [qoff[c]]: the bits of every query's minimum
    UhdRec *recs;                  // [items]
    double *out_d2;                // [c]
    int *out_ij;                   // [c, 2]
};
static_assert(sizeof(UhdRaggedArgs) <= 4096, "the pair table must fit the kernel arguments");

__global__ __launch_bounds__(kUhdBlock) void uhd_ragged_init_kernel(int total, unsigned long long *__restrict__ qmin)
{
    const int i = blockIdx.x * kUhdBlock + threadIdx.x;
    if (i < total) qmin[i] = kUhdInfBits;
}

__global__ __launch_bounds__(kUhdBlock) void uhd_ragged_pairs_kernel(UhdRaggedArgs a)
{
    __shared__ double s_t[kUhdTile * 3];
    const int item = blockIdx.x;
    const int pair = ragged_pair_of_shift(a.t, item, kUhdRaggedShift);
    const int q0 = a.t.qoff[pair], n = a.t.qoff[pair + 1] - q0;
    const int t0 = a.t.toff[pair], m = a.t.toff[pair + 1] - t0;
    const long long base = ragged_item_base_shift(a.t, pair, item, kUhdRaggedShift);
    const long long j0 = (long long)blockIdx.y * kUhdTile;
    if (base >= n || j0 >= m) return;                              // (uniform: the whole workgroup leaves)
    const int cnt = min(kUhdTile, m - (int)j0);
    const float *__restrict__ T = a.tg + ((size_t)t0 + (size_t)j0) * 3;
    for (int k = threadIdx.x; k < cnt * 3; k += kUhdBlock) s_t[k] = (double)T[k];
    __syncthreads();
    const int i0 = (int)base + threadIdx.x;
    const float *__restrict__ Q = a.q + (size_t)q0 * 3;
    double qx[kUhdQ], qy[kUhdQ], qz[kUhdQ], best[kUhdQ];
#pragma unroll
    for (int q = 0; q < kUhdQ; q++) {
        const int i = min(i0 + q * kUhdBlock, n - 1);          // lanes past the end redo the last query and store nothing
        qx[q] = (double)Q[(size_t)i * 3 + 0];
        qy[q] = (double)Q[(size_t)i * 3 + 1];
        qz[q] = (double)Q[(size_t)i * 3 + 2];
        best[q] = __builtin_inf();
    }
#pragma unroll 4
    for (int j = 0; j < cnt; j++) {
        const double tx = s_t[j * 3 + 0], ty = s_t[j * 3 + 1], tz = s_t[j * 3 + 2];
#pragma unroll
        for (int q = 0; q < kUhdQ; q++) best[q] = fmin(best[q], uhd_s(qx[q], qy[q], qz[q], tx, ty, tz));
    }
    unsigned long long *__restrict__ W = a.qmin + q0;
#pragma unroll
    for (int q = 0; q < kUhdQ; q++) {
        const int i = i0 + q * kUhdBlock;
        if (i < n) atomicMin(&W[i], (unsigned long long)__double_as_longlong(best[q]));
    }
}

__global__ __launch_bounds__(kUhdBlock) void uhd_ragged_query_kernel(UhdRaggedArgs a)
{
    __shared__ UhdRec s_r[kUhdBlock];
    const int item = blockIdx.x;
    const int pair = ragged_pair_of_shift(a.t, item, kUhdRaggedShift);
    const int q0 = a.t.qoff[pair], n = a.t.qoff[pair + 1] - q0;
    const long long base = ragged_item_base_shift(a.t, pair, item, kUhdRaggedShift);
    UhdRec r{-1.0, kUhdNoIndex, 0};                    // below every minimum (s >= 0): an idle item's record, too
    if (base < n) {
        const unsigned long long *__restrict__ W = a.qmin + q0;
#pragma unroll
        for (int q = 0; q < kUhdQ; q++) {              // ascending i: a later one must be strictly greater to win
            const int i = (int)base + q * kUhdBlock + threadIdx.x;
            if (i < n) {
                const double v = __longlong_as_double((long long)W[i]);
                if (uhd_beats(v, i, r.v, r.i)) r = UhdRec{v, i, 0};
            }
        }
    }
    r = uhd_block_best(r, s_r);
    if (threadIdx.x == 0) a.recs[item] = r;
}

__global__ __launch_bounds__(kUhdBlock) void uhd_ragged_finish_kernel(UhdRaggedArgs a)
{
    __shared__ UhdRec s_r[kUhdBlock];
    __shared__ int s_j[kUhdBlock];
    const int pair = blockIdx.x;
    const int q0 = a.t.qoff[pair], n = a.t.qoff[pair + 1] - q0;
    const int t0 = a.t.toff[pair], m = a.t.toff[pair + 1] - t0;
    const int first = ragged_first_item_shift(a.t, pair, kUhdRaggedShift);
    const int nrecs = (int)(((long long)n + (1 << kUhdRaggedShift) - 1) >> kUhdRaggedShift);
    UhdRec r{-1.0, kUhdNoIndex, 0};
    for (int k = threadIdx.x; k < nrecs; k += kUhdBlock) {
        const UhdRec o = a.recs[first + k];
        if (uhd_beats(o.v, o.i, r.v, r.i)) r = o;
    }
    r = uhd_block_best(r, s_r);
    const float *qp = a.q + ((size_t)q0 + min(r.i, n - 1)) * 3;             // (r.i is a query index: the pair has a query)
    const double qx = (double)qp[0], qy = (double)qp[1], qz = (double)qp[2];
    const float *__restrict__ T = a.tg + (size_t)t0 * 3;
    int jbest = kUhdNoIndex;
    for (int k = threadIdx.x; k < m; k += kUhdBlock) {                       // ascending per thread: the first hit is the thread's lowest
        const float *tp = T + (size_t)k * 3;
        if (uhd_s(qx, qy, qz, (double)tp[0], (double)tp[1], (double)tp[2]) == r.v) { jbest = k; break; }
    }
    s_j[threadIdx.x] = jbest;
    __syncthreads();
    for (int w = kUhdBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s_j[threadIdx.x] = min(s_j[threadIdx.x], s_j[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        a.out_d2[pair] = r.v;
        a.out_ij[pair * 2 + 0] = r.i;
        a.out_ij[pair * 2 + 1] = s_j[0] == kUhdNoIndex ? -1 : s_j[0];
    }
}

static int uhd_ragged(const RaggedTable &t, int max_targets, const float *xyz, const float *xyz2, double *out_d2, int *out_ij, hipStream_t st)
{
    const int c = t.c, total = t.qoff[c];
    const int items = (int)ragged_items_shift(total, c, kUhdRaggedShift), tiles = ceil_div(max_targets, kUhdTile);
    if (tiles > 65535) {
        set_error("genpc_uhd_ragged: problem too large for one launch (every pair's M <= 65535 * 512)");
        return -1;
    }
    UhdRaggedArgs a{};
    a.t = t; a.q = xyz; a.tg = xyz2; a.out_d2 = out_d2; a.out_ij = out_ij;
    WsLayout L;
    L.add(a.qmin, (size_t)total);
    L.add(a.recs, (size_t)items);
    if (!ws_alloc(L, kWsUhdRagged, st)) return -1;
    hipLaunchKernelGGL(uhd_ragged_init_kernel, dim3(ceil_div(total, kUhdBlock)), dim3(kUhdBlock), 0, st, total, a.qmin);
    if (!check(hipGetLastError(), "uhd_ragged_init_kernel launch")) return -1;
    hipLaunchKernelGGL(uhd_ragged_pairs_kernel, dim3(items, tiles), dim3(kUhdBlock), 0, st, a);
    if (!check(hipGetLastError(), "uhd_ragged_pairs_kernel launch")) return -1;
    hipLaunchKernelGGL(uhd_ragged_query_kernel, dim3(items), dim3(kUhdBlock), 0, st, a);
    if (!check(hipGetLastError(), "uhd_ragged_query_kernel launch")) return -1;
    hipLaunchKernelGGL(uhd_ragged_finish_kernel, dim3(c), dim3(kUhdBlock), 0, st, a);
    return check(hipGetLastError(), "uhd_ragged_finish_kernel launch") ? 0 : -1;
}

}  // namespace genpc

GENPC_API int genpc_uhd_ragged(int c, const int *noff, const float *xyz, const int *moff, const float *xyz2, double *out_d2, int *out_ij,
                               void *stream)
{
    using namespace genpc;
    RaggedTable t;
    int max_targets = 0;
    const char *err = nullptr;
    const int rc = ragged_table_fill(c, noff, moff, t, &max_targets, &err);
    if (rc < 0) return ragged_refuse("genpc_uhd_ragged", err);
    if (c == 0) return 1;
    for (int j = 0; j < c; j++) {              // (rc == 0 with c > 0: no pair has a query)
        if (noff[j + 1] == noff[j] || moff[j + 1] == moff[j]) {
            char msg[160];
            snprintf(msg, sizeof msg, "genpc_uhd_ragged: pair %d has no %s (the maximum or minimum of an empty set is undefined)", j,
                     noff[j + 1] == noff[j] ? "queries" : "targets");
            set_error(msg);
            return -1;
        }
    }
    if (!xyz || !xyz2 || !out_d2 || !out_ij) {
        set_error("genpc_uhd_ragged: null pointer");
        return -1;
    }
    return uhd_ragged(t, max_targets, xyz, xyz2, out_d2, out_ij, (hipStream_t)stream);
}
