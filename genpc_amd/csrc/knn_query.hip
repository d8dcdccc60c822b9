// knn_query.hip -- the exact k nearest targets of every query, with their indices (1 <= k <= 32).
//
// The reference densifies the partial scan before stage 1 with a KD-tree query of k = 2 or 5 neighbours and inverse-distance
// weights (utils/dataUtils.py:128-134); every other search of the library answers "which target is nearest" only, and
// knn.hip returns a mean distance inside one cloud.  Here queries [B, NQ, 3] meet targets [B, NT, 3]:
//   * the targets are sorted once per call into the x-fastest grid of grid.h (launch_cell_grid_build): the cells
//     [x0, x1] of a (cy, cz) row are one contiguous run of `sorted`;
//   * the query ids are sorted by their cell in the TARGET grid (knn_query_order_kernel, the counting-sort pieces of grid.h),
//     so the 64 lanes of a wave walk neighbouring cells;
//   * one lane owns a query.  Its k best candidates live in registers as an ascending list of the 64-bit keys
//     distance bits << 32 | target index (nn_grid.hip's): distances ascend, among bit-equal distances the lower index comes
//     first, and the same order decides which of several equal candidates holds the k-th place.  The list has CAP entries
//     (4, 8, 16 or 32, the next capacity above k); its first CAP - k entries are pinned to key 0, below every candidate, so
//     the k-th best is always the LAST entry and the call's k results are the last k;
//   * the lane visits the targets by grid.h's cell_grid_shell_walk, which skips and stops against that k-th best;
//   * the distance is sqdist<FMA> of common.h in the call's arithmetic mode: column 0 holds the bits of genpc_nm_distance.
//     Only candidates with d < +inf are listed (NaN and infinite distances never enter); slots past the listed ones hold
//     (+inf, -1).  A target cloud with a non-finite coordinate (CellGridHdr.bad) is searched without culling.
// One path for every size: a tiny or degenerate cloud is a one-cell grid.
//
// The ragged form (genpc_knn_query_ragged): c (queries, targets) pairs of any sizes, packed, one call, three launches.
//   * grid.hip's ragged build sorts every pair's targets into a grid of their own (ragged_table.h).  Its cells are sized for
//     k <= 5 whatever k is; the search is exact on any grid, so a pair's rows are the bits of genpc_knn_query on it alone.
//   * knn_query_order_ragged_kernel: one workgroup per pair, the same counting sort (knn_query_order_of, one body for both
//     kernels); order[qoff[j] + .] holds query ids inside pair j.
//   * knn_query_ragged_kernel: the same search (knn_query_of, one body for both kernels).  A workgroup serves up to 256 sorted
//     queries of ONE pair: blockIdx.x is a work item of ragged_items.h's numbering with shift 8, the pair comes from a binary
//     search of the table in the kernel arguments (uniform: scalar loads).
#include "nn.h"
#include "ragged_items.h"
#include "../../include/genpc_hip.h"

namespace genpc {

constexpr int kKQOBlock = 1024;                                  // query ordering: one block per batch element
constexpr unsigned long long kKQEmpty = 0x7f800000ffffffffull;   // (+inf, -1): above every listed candidate

struct KnnQueryArgs {
    const float *q;            // [b][nq][3]
    const float4 *sorted;      // [b][nt]: (x, y, z, index) in cell order
    const int *start;          // [b][cells_max + 1]
    const CellGridHdr *hdr;    // [b]
    const int *order;          // [b][nq]: query ids by cell of the target grid
    float *out_d;              // [b][nq][k]
    int *out_i;
    int nq, nt, k, cells_max, qblocks;
};

// THE ordering of one cloud's queries (knn_query_order_kernel, knn_query_order_ragged_kernel): O[.] = the ids of the nq
// queries Q sorted by their cell in the target grid H (a counting sort in LDS; the order inside a cell is whatever the atomics
// give: every query writes its own results, so it reaches none of them).  The whole workgroup calls it.
__device__ __forceinline__ void knn_query_order_of(int nq, const float *__restrict__ Q, const CellGridHdr &H, int *__restrict__ O, int *s_cnt,
                                                   int *s_w)
{
    for (int i = threadIdx.x; i < H.cells; i += kKQOBlock) s_cnt[i] = 0;
    __syncthreads();
    auto cell_of = [&](int j) {
        const int cx = grid_cell1(Q[(size_t)j * 3 + 0], H.lo[0], H.inv, H.g[0]), cy = grid_cell1(Q[(size_t)j * 3 + 1], H.lo[1], H.inv, H.g[1]);
        const int cz = grid_cell1(Q[(size_t)j * 3 + 2], H.lo[2], H.inv, H.g[2]);
        return (cz * H.g[1] + cy) * H.g[0] + cx;
    };
    for (int j = threadIdx.x; j < nq; j += kKQOBlock) atomicAdd(&s_cnt[cell_of(j)], 1);
    __syncthreads();
    grid_scan_counts<kKQOBlock>(s_cnt, H.cells, 0, s_w);
    for (int j = threadIdx.x; j < nq; j += kKQOBlock) O[atomicAdd(&s_cnt[cell_of(j)], 1)] = j;
}

// order[batch][.] = the query ids of a batch element sorted by their cell in the element's target grid
__global__ __launch_bounds__(kKQOBlock) void knn_query_order_kernel(int nq, const float *__restrict__ q, const CellGridHdr *__restrict__ hdr,
                                                                    int *__restrict__ order, int cells_max)
{
    extern __shared__ int s_cnt[];            // cells_max counters, then 2 ints per wave
    const int batch = blockIdx.x;
    const CellGridHdr H = hdr[batch];
    knn_query_order_of(nq, q + (size_t)batch * nq * 3, H, order + (size_t)batch * nq, s_cnt, s_cnt + cells_max);
}

// THE search of one query (knn_query_kernel, knn_query_ragged_kernel): the target cloud's grid (H, its cell table ST, its sorted
// points S), the query and the k slots od / oi of its results.
template <int CAP, int FMA>
__device__ __forceinline__ void knn_query_of(const CellGridHdr &H, const float4 *__restrict__ S, const int *__restrict__ ST, const float qx,
                                             const float qy, const float qz, const int k, float *__restrict__ od, int *__restrict__ oi)
{
    unsigned long long L[CAP];           // ascending; L[0 .. CAP - k) pinned to 0, L[CAP - 1] is the k-th best
#pragma unroll
    for (int i = 0; i < CAP; i++) L[i] = i < CAP - k ? 0ull : kKQEmpty;
    auto kth = [&]() { return __uint_as_float((unsigned)(L[CAP - 1] >> 32)); };      // +inf while fewer than k are listed
    auto run = [&](int p0, int p1) {     // the targets at positions [p0, p1) of the sorted cloud
        for (int p = p0; p < p1; p++) {
            const float4 e = S[p];
            const float dd = sqdist<FMA>(e.x - qx, e.y - qy, e.z - qz);
            const unsigned long long key = ((unsigned long long)__float_as_uint(dd) << 32) | (unsigned)__float_as_int(e.w);
            if (dd < __builtin_inff() && key < L[CAP - 1]) {
                // sorted insertion, the largest falls off:  L'[i] = max(L[i - 1], min(key, L[i]))
#pragma unroll
                for (int i = CAP - 1; i > 0; i--) {
                    const unsigned long long m = key < L[i] ? key : L[i];
                    L[i] = L[i - 1] > m ? L[i - 1] : m;
                }
                L[0] = key < L[0] ? key : L[0];
            }
        }
    };

    cell_grid_shell_walk(H, ST, qx, qy, qz, kth, run);
    const int skip = CAP - k;
#pragma unroll
    for (int i = 0; i < CAP; i++) {
        if (i >= skip) {
            od[i - skip] = __uint_as_float((unsigned)(L[i] >> 32));
            oi[i - skip] = (int)(unsigned)L[i];
        }
    }
}

template <int CAP, int FMA>
__global__ __launch_bounds__(kBlock) void knn_query_kernel(KnnQueryArgs a)
{
    const int batch = blockIdx.x / a.qblocks, pos = (blockIdx.x - batch * a.qblocks) * kBlock + threadIdx.x;
    if (pos >= a.nq) return;
    const int j = a.order[(size_t)batch * a.nq + pos];
    const float *qp = a.q + ((size_t)batch * a.nq + j) * 3;
    const float qx = qp[0], qy = qp[1], qz = qp[2];
    const float4 *__restrict__ S = a.sorted + (size_t)batch * a.nt;
    const int *__restrict__ ST = a.start + (size_t)batch * (a.cells_max + 1);
    const CellGridHdr H = a.hdr[batch];
    knn_query_of<CAP, FMA>(H, S, ST, qx, qy, qz, a.k, a.out_d + ((size_t)batch * a.nq + j) * a.k, a.out_i + ((size_t)batch * a.nq + j) * a.k);
}

template <int CAP>
static void launch_knn_query_cap(const KnnQueryArgs &a, unsigned grid, int fma, hipStream_t st)
{
    if (fma) hipLaunchKernelGGL((knn_query_kernel<CAP, 1>), dim3(grid), dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((knn_query_kernel<CAP, 0>), dim3(grid), dim3(kBlock), 0, st, a);
}

static int knn_query(int b, int nq, const float *xyz, int nt, const float *xyz2, int k, float *dist, int *idx, hipStream_t st)
{
    const int fma = arith_mode() != 0;
    KnnQueryArgs a{};
    a.q = xyz; a.out_d = dist; a.out_i = idx; a.nq = nq; a.nt = nt; a.k = k; a.cells_max = kCellGridMaxCells;
    WsLayout L;
    L.add(a.hdr, b);
    L.add(a.start, (size_t)b * (kCellGridMaxCells + 1));
    L.add(a.sorted, (size_t)b * nt);
    L.add(a.order, (size_t)b * nq);
    if (!ws_alloc(L, kWsKnnQuery, st)) return 0;
    a.qblocks = ceil_div(nq, kBlock);
    if ((long long)b * a.qblocks > 0x7fffffffLL) { set_error("knn query: problem too large for one launch"); return 0; }
    // cells of about max(2, k / 2) targets: the 27 cells around a query then hold its k neighbours more often than not
    const int per = k / 2 > 2 ? k / 2 : 2;
    int target = nt / per;
    target = target < 8 ? 8 : (target > kCellGridMaxCells * 3 / 4 ? kCellGridMaxCells * 3 / 4 : target);
    if (!launch_cell_grid_build(b, nt, xyz2, nullptr, (CellGridHdr *)a.hdr, (int *)a.start, (float4 *)a.sorted, nullptr, nullptr, target,
                                kCellGridMaxCells, st))
        return 0;
    const size_t lds = ((size_t)kCellGridMaxCells + 2 * (kKQOBlock / kWave)) * sizeof(int);
    hipLaunchKernelGGL(knn_query_order_kernel, dim3(b), dim3(kKQOBlock), lds, st, nq, xyz, a.hdr, (int *)a.order, kCellGridMaxCells);
    if (!check(hipGetLastError(), "knn_query_order_kernel launch")) return 0;
    const unsigned grid = (unsigned)(b * a.qblocks);
    if (k <= 4) launch_knn_query_cap<4>(a, grid, fma, st);
    else if (k <= 8) launch_knn_query_cap<8>(a, grid, fma, st);
    else if (k <= 16) launch_knn_query_cap<16>(a, grid, fma, st);
    else launch_knn_query_cap<32>(a, grid, fma, st);
    return check(hipGetLastError(), "knn_query_kernel launch") ? 1 : 0;
}

// ---- the ragged form ----
constexpr int kKQRShift = 8;                      // a work item: kBlock sorted queries of one pair
static_assert((1 << kKQRShift) == kBlock, "a work item is what a workgroup of the search owns");

struct KnnQueryRaggedArgs {
    RaggedTable t;
    const float *q;                // packed queries
    const float4 *sorted;          // packed, every pair's targets in their own cell order: (x, y, z, index inside the pair's cloud)
    const int *start;              // pair j's cell table at toff[j] + 65 j
    const CellGridHdr *hdr;        // [c]
    const int *order;              // packed like the queries: query ids INSIDE the pair, by cell of the pair's target grid
    float *out_d;                  // [queries][k], packed like the queries
    int *out_i;
    int k;
};
static_assert(sizeof(KnnQueryRaggedArgs) <= 4096, "the pair table must fit the kernel arguments");

// one workgroup per pair
__global__ __launch_bounds__(kKQOBlock) void knn_query_order_ragged_kernel(RaggedTable t, const float *__restrict__ q,
                                                                           const CellGridHdr *__restrict__ hdr, int *__restrict__ order,
                                                                           int lds_cells)
{
    extern __shared__ int s_cnt[];            // lds_cells counters, then 2 ints per wave
    const int pair = blockIdx.x;
    const int q0 = t.qoff[pair], nq = t.qoff[pair + 1] - q0;
    if (nq == 0) return;                      // nobody asks: no grid was built (the whole block leaves: no barrier is left waiting)
    const CellGridHdr H = hdr[pair];
    knn_query_order_of(nq, q + (size_t)q0 * 3, H, order + q0, s_cnt, s_cnt + lds_cells);
}

template <int CAP, int FMA>
__global__ __launch_bounds__(kBlock) void knn_query_ragged_kernel(KnnQueryRaggedArgs a)
{
    const int item = blockIdx.x;
    const int pair = ragged_pair_of_shift(a.t, item, kKQRShift);
    const int q0 = a.t.qoff[pair], nq = a.t.qoff[pair + 1] - q0, t0 = a.t.toff[pair];
    const long long pos = ragged_item_base_shift(a.t, pair, item, kKQRShift) + threadIdx.x;
    if (pos >= nq) return;
    const int j = a.order[(size_t)q0 + pos];
    const float *qp = a.q + ((size_t)q0 + j) * 3;
    const float qx = qp[0], qy = qp[1], qz = qp[2];
    const float4 *__restrict__ S = a.sorted + t0;
    const int *__restrict__ ST = a.start + ((size_t)t0 + (size_t)kRaggedStartPad * pair);
    const CellGridHdr H = a.hdr[pair];
    knn_query_of<CAP, FMA>(H, S, ST, qx, qy, qz, a.k, a.out_d + ((size_t)q0 + j) * a.k, a.out_i + ((size_t)q0 + j) * a.k);
}

template <int CAP>
static void launch_knn_query_ragged_cap(const KnnQueryRaggedArgs &a, unsigned grid, int fma, hipStream_t st)
{
    if (fma) hipLaunchKernelGGL((knn_query_ragged_kernel<CAP, 1>), dim3(grid), dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((knn_query_ragged_kernel<CAP, 0>), dim3(grid), dim3(kBlock), 0, st, a);
}

static int knn_query_ragged(int c, const int *noff, const int *moff, const float *xyz, const float *xyz2, int k, float *dist, int *idx,
                            hipStream_t st)
{
    if (k < 1 || k > 32) {
        set_error("genpc_knn_query_ragged: k must be 1 .. 32");
        return -1;
    }
    KnnQueryRaggedArgs a{};
    int max_targets = 0;
    const char *err = nullptr;
    const int rc = ragged_table_fill(c, noff, moff, a.t, &max_targets, &err);
    if (rc < 0) return ragged_refuse("genpc_knn_query_ragged", err);
    if (rc == 0) return 1;
    if (!xyz || !xyz2 || !dist || !idx) {
        set_error("genpc_knn_query_ragged: null pointer");
        return -1;
    }
    const int fma = arith_mode() != 0;
    const int queries = a.t.qoff[c], targets = a.t.toff[c];
    a.q = xyz; a.out_d = dist; a.out_i = idx; a.k = k;
    WsLayout L;
    L.add(a.hdr, c);
    L.add(a.start, (size_t)ragged_start_len(targets, c));
    L.add(a.sorted, (size_t)targets);
    L.add(a.order, (size_t)queries);
    if (!ws_alloc(L, kWsKnnQueryRagged, st)) return 0;
    if (!launch_cell_grid_build_ragged(a.t, max_targets, xyz2, (CellGridHdr *)a.hdr, (int *)a.start, (float4 *)a.sorted, st)) return 0;
    const int lds_cells = ragged_cells_max(max_targets);       // every built grid has at most this many cells
    const size_t lds = ((size_t)lds_cells + 2 * (kKQOBlock / kWave)) * sizeof(int);
    hipLaunchKernelGGL(knn_query_order_ragged_kernel, dim3(c), dim3(kKQOBlock), lds, st, a.t, xyz, a.hdr, (int *)a.order, lds_cells);
    if (!check(hipGetLastError(), "knn_query_order_ragged_kernel launch")) return 0;
    const unsigned grid = (unsigned)ragged_items_shift(queries, c, kKQRShift);
    if (k <= 4) launch_knn_query_ragged_cap<4>(a, grid, fma, st);
    else if (k <= 8) launch_knn_query_ragged_cap<8>(a, grid, fma, st);
    else if (k <= 16) launch_knn_query_ragged_cap<16>(a, grid, fma, st);
    else launch_knn_query_ragged_cap<32>(a, grid, fma, st);
    return check(hipGetLastError(), "knn_query_ragged_kernel launch") ? 1 : 0;
}

}  // namespace genpc

GENPC_API int genpc_knn_query(int b, int nq, const float *xyz, int nt, const float *xyz2, int k, float *dist, int *idx, void *stream)
{
    using namespace genpc;
    if (k < 1 || k > 32) {
        set_error("genpc_knn_query: k must be 1 .. 32");
        return -1;
    }
    if (b < 0 || nq < 0 || nt < 0) {
        set_error("genpc_knn_query: negative size");
        return -1;
    }
    if (b == 0 || nq == 0) return 1;
    if (nt < 1) {
        set_error("genpc_knn_query: no targets");
        return -1;
    }
    return knn_query(b, nq, xyz, nt, xyz2, k, dist, idx, (hipStream_t)stream);
}

GENPC_API int genpc_knn_query_ragged(int c, const int *noff, const float *xyz, const int *moff, const float *xyz2, int k, float *dist, int *idx,
                                     void *stream)
{
    return genpc::knn_query_ragged(c, noff, moff, xyz, xyz2, k, dist, idx, (hipStream_t)stream);
}
