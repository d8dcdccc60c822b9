// probe.hip -- hardware-premise probes the test-suite runs on the box it is on:
// the f16 MFMA's summation error (below) and fastdiv.h's shared-reciprocal division against the compiler's.
//
// The default NN path (nn_f16.hip) evaluates |t|^2 - 2 q.t for 32 x 32 pairs with ONE
// v_mfma_f32_32x32x16_f16 and proves its candidate lists complete from a bound on that instruction's K = 16
// summation error: |result - exact| <= 6.5 u sum|terms| (u = 2^-24; measured 3.1 u on the development box,
// tools/ubench_mfma_f16.hip).  The bound is a property of the matrix pipe's internal accumulation, which no
// document states: genpc_mfma_f16_probe runs the instruction on caller-supplied operands so that
// tests/test_gpu_mfma_premise.py can re-measure it wherever the suite runs -- a stepping that accumulates
// differently fails a test instead of silently corrupting nearest neighbours.
// Further down: grid.h's cell function, sizing, skip bound and cell range and grid.hip's two builds on caller-supplied inputs
// (tests/test_gpu_grid.py) -- the same idea for arithmetic the library proves on paper.
#include "nn.h"
#include "fastdiv.h"
#include "grid.h"
#include "../../include/genpc_hip.h"

#include <stdint.h>

namespace genpc {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// One wave per problem: D[32,32] = A[32,16] * B[16,32] + C[32,32] (A, B f16 bit patterns, row-major).
// Lane l supplies A[l&31][8*(l>>5) .. +7] and B[8*(l>>5) .. +7][l&31]; D[i][j]: lane j + 32*((i>>2)&1), register
// (i>>3)*4 + (i&3) -- the operand layout nn_f16_kernel uses.
__global__ __launch_bounds__(kWave) void mfma_f16_probe_kernel(const uint16_t *__restrict__ A, const uint16_t *__restrict__ B,
                                                               const float *__restrict__ C, float *__restrict__ D)
{
    const int l = threadIdx.x;
    A += (size_t)blockIdx.x * 32 * 16;
    B += (size_t)blockIdx.x * 16 * 32;
    C += (size_t)blockIdx.x * 32 * 32;
    D += (size_t)blockIdx.x * 32 * 32;
    s16x8 as, bs;
    for (int k = 0; k < 8; k++) {
        as[k] = (short)A[(l & 31) * 16 + 8 * (l >> 5) + k];
        bs[k] = (short)B[(8 * (l >> 5) + k) * 32 + (l & 31)];
    }
    f32x16 c;
    for (int r = 0; r < 16; r++) c[r] = C[((r >> 2) * 8 + (l >> 5) * 4 + (r & 3)) * 32 + (l & 31)];
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, as), __builtin_bit_cast(h16x8, bs), c, 0, 0, 0);
    for (int r = 0; r < 16; r++) D[((r >> 2) * 8 + (l >> 5) * 4 + (r & 3)) * 32 + (l & 31)] = c[r];
}

// fastdiv.h against the compiler's division, element by element: fast[i] = div_core(num[i], den[i], rcp_refined(den[i])),
// the packed form with the pair (i, i ^ 1), ieee[i] = num[i] / den[i], in_range[i] = what the callers' range test says.
__global__ __launch_bounds__(256) void fastdiv_probe_kernel(long long n, const float *__restrict__ num, const float *__restrict__ den,
                                                            float *__restrict__ fast, float *__restrict__ fast2,
                                                            float *__restrict__ ieee, unsigned char *__restrict__ in_range)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float a = num[i], d = den[i];
        const long long j = (i ^ 1) < n ? (i ^ 1) : i;
        const float a2 = num[j], d2 = den[j];
        fast[i] = div_core(a, d, rcp_refined(d));
        const v2f q = div_core2((v2f){a, a2}, (v2f){d, d2}, (v2f){rcp_refined(d), rcp_refined(d2)});
        fast2[i] = q.x;
        ieee[i] = a / d;
        DivRange r;
        r.add(a, d);
        in_range[i] = r.ok() ? 1 : 0;
    }
}

// the list hand-off's coded lower bounds (nn.h): out[i] = list_dec(base[i], list_enc(base[i], v[i]))
__global__ __launch_bounds__(256) void list_code_probe_kernel(long long n, const float *__restrict__ base, const float *__restrict__ v,
                                                              float *__restrict__ out)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        out[i] = list_dec(base[i], list_enc(base[i], v[i]));
}

// ---- grid.h / grid.hip under test (tests/test_gpu_grid.py): the kernels below call the helpers themselves and restate nothing ----
static_assert(sizeof(GridFrame) == 11 * 4 && sizeof(CellGridHdr) == 13 * 4, "include/genpc_hip.h documents the header's words");

// one thread per box: frames[i] = grid_size<16, false> or <12, true> of (mn[i], mx[i])
__global__ __launch_bounds__(256) void grid_size_probe_kernel(int nbox, int coarse, const float *__restrict__ mn, const float *__restrict__ mx,
                                                              const int *__restrict__ cells_target, const int *__restrict__ cells_max,
                                                              GridFrame *__restrict__ frames)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nbox) return;
    float a[3] = {mn[i * 3 + 0], mn[i * 3 + 1], mn[i * 3 + 2]}, b[3] = {mx[i * 3 + 0], mx[i * 3 + 1], mx[i * 3 + 2]};
    GridFrame F;
    if (coarse) grid_size<12, true>(a, b, cells_target[i], cells_max[i], F);
    else grid_size<16, false>(a, b, cells_target[i], cells_max[i], F);
    frames[i] = F;
}

// the cell of every query and point per axis, and every query's slack per axis
__global__ __launch_bounds__(256) void grid_cell_probe_kernel(const GridFrame *__restrict__ hdr, int nq, const float *__restrict__ q, int n,
                                                              const float *__restrict__ p, int *__restrict__ qcell, int *__restrict__ pcell,
                                                              float *__restrict__ qslack)
{
    const GridFrame F = *hdr;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < 3ll * (nq + n); i += (long long)gridDim.x * 256) {
        const int a = (int)(i % 3);
        const long long j = i / 3;
        if (j < nq) {
            qcell[i] = grid_cell1(q[i], F.lo[a], F.inv, F.g[a]);
            qslack[i] = grid_slack(F.slack[a], q[i]);
        } else {
            pcell[i - 3ll * nq] = grid_cell1(p[i - 3ll * nq], F.lo[a], F.inv, F.g[a]);
        }
    }
}

// slab[((j * 3 + a) * gmax + c) * 2 + {0, 1}] = the shell walk's two slab gaps of query j on axis a beyond cell c, cells [0, c)
// and [c, g); slabb: (m * m) * kGridShrink of each
__global__ __launch_bounds__(256) void grid_slab_probe_kernel(const GridFrame *__restrict__ hdr, int nq, const float *__restrict__ q, int gmax,
                                                              const float *__restrict__ mn, const float *__restrict__ mx,
                                                              float *__restrict__ slab, float *__restrict__ slabb)
{
    const GridFrame F = *hdr;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < 3ll * nq * gmax; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % gmax), a = (int)((i / gmax) % 3);
        const long long j = i / gmax / 3;
        const int g = F.g[a];
        if (c >= g) continue;
        const float qa = q[j * 3 + a], s = grid_slack(F.slack[a], qa);
        const float m0 = mn ? grid_gap(0, c, g, F.lo[a], F.h, qa, s, mn[a], mx[a]) : grid_gap(0, c, g, F.lo[a], F.h, qa, s);
        const float m1 = mn ? grid_gap(c, g - c, g, F.lo[a], F.h, qa, s, mn[a], mx[a]) : grid_gap(c, g - c, g, F.lo[a], F.h, qa, s);
        slab[i * 2 + 0] = m0;
        slab[i * 2 + 1] = m1;
        slabb[i * 2 + 0] = __fmul_rn(m0, m0) * kGridShrink;
        slabb[i * 2 + 1] = __fmul_rn(m1, m1) * kGridShrink;
    }
}

// pair (j, i) of query j and point i: gap1 / gap4 [pair][3] = grid_gap of the point's cell (w = 1) and of its aligned block of
// four cells (nn_grid.hip's coarse_lb), bound[pair][3] = the shrunk bounds as the consumers associate them (all axes w = 1,
// y and z only w = 1, all axes w = 4), sq[pair][2] = sqdist<0>, sqdist<1> of point - query
__global__ __launch_bounds__(256) void grid_pair_probe_kernel(const GridFrame *__restrict__ hdr, int nq, const float *__restrict__ q, int n,
                                                              const float *__restrict__ p, const float *__restrict__ mn,
                                                              const float *__restrict__ mx, float *__restrict__ gap1, float *__restrict__ gap4,
                                                              float *__restrict__ bound, float *__restrict__ sq)
{
    const GridFrame F = *hdr;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < (long long)nq * n; t += (long long)gridDim.x * 256) {
        const long long j = t / n, i = t % n;
        float g1[3], g4[3], d[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float qa = q[j * 3 + a], pa = p[i * 3 + a], s = grid_slack(F.slack[a], qa);
            const int g = F.g[a], c = grid_cell1(pa, F.lo[a], F.inv, g), C = c >> 2;
            g1[a] = mn ? grid_gap(c, 1, g, F.lo[a], F.h, qa, s, mn[a], mx[a]) : grid_gap(c, 1, g, F.lo[a], F.h, qa, s);
            g4[a] = mn ? grid_gap(C * 4, 4, g, F.lo[a], F.h, qa, s, mn[a], mx[a]) : grid_gap(C * 4, 4, g, F.lo[a], F.h, qa, s);
            d[a] = pa - qa;
            gap1[t * 3 + a] = g1[a];
            gap4[t * 3 + a] = g4[a];
        }
        bound[t * 3 + 0] = __fmaf_rn(g1[0], g1[0], __fmaf_rn(g1[1], g1[1], __fmul_rn(g1[2], g1[2]))) * kGridShrink;
        bound[t * 3 + 1] = __fmaf_rn(g1[1], g1[1], __fmul_rn(g1[2], g1[2])) * kGridShrink;
        bound[t * 3 + 2] = __fmaf_rn(g4[0], g4[0], __fmaf_rn(g4[1], g4[1], __fmul_rn(g4[2], g4[2]))) * kGridShrink;
        sq[t * 2 + 0] = sqdist<0>(d[0], d[1], d[2]);
        sq[t * 2 + 1] = sqdist<1>(d[0], d[1], d[2]);
    }
}

// range[(j * 3 + a) * 2 + {0, 1}] = grid_cell_range of query j on axis a with radius R[j * 3 + a]; with b01 != null the
// range clipped to [b01[.. * 2], b01[.. * 2 + 1]] by grid_cell_range_in
__global__ __launch_bounds__(256) void grid_range_probe_kernel(const GridFrame *__restrict__ hdr, int nq, const float *__restrict__ q,
                                                               const float *__restrict__ R, const int *__restrict__ b01, int *__restrict__ range)
{
    const GridFrame F = *hdr;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < 3ll * nq; i += (long long)gridDim.x * 256) {
        const int a = (int)(i % 3);
        const float s = grid_slack(F.slack[a], q[i]);
        const GridRange r = b01 ? grid_cell_range_in(q[i], R[i], s, F.lo[a], F.inv, F.g[a], b01[i * 2], b01[i * 2 + 1])
                                : grid_cell_range(q[i], R[i], s, F.lo[a], F.inv, F.g[a]);
        range[i * 2 + 0] = r.c0;
        range[i * 2 + 1] = r.c1;
    }
}

}  // namespace genpc

GENPC_API int genpc_list_code_probe(long long n, const float *base, const float *v, float *out, void *stream)
{
    using namespace genpc;
    if (n < 0) return -1;
    if (n == 0) return 1;
    const long long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(list_code_probe_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, n, base,
                       v, out);
    return check(hipGetLastError(), "list code probe launch") ? 1 : 0;
}

GENPC_API int genpc_fastdiv_probe(long long n, const float *num, const float *den, float *fast, float *fast_packed, float *ieee,
                                  unsigned char *in_range, void *stream)
{
    using namespace genpc;
    if (n < 0) return -1;
    if (n == 0) return 1;
    const long long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(fastdiv_probe_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, n, num,
                       den, fast, fast_packed, ieee, in_range);
    return check(hipGetLastError(), "fastdiv probe launch") ? 1 : 0;
}

GENPC_API int genpc_mfma_f16_probe(int problems, const unsigned short *a, const unsigned short *b, const float *c, float *d,
                                   void *stream)
{
    using namespace genpc;
    if (problems < 0) return -1;
    if (problems == 0) return 1;
    hipLaunchKernelGGL(mfma_f16_probe_kernel, dim3(problems), dim3(kWave), 0, (hipStream_t)stream, (const uint16_t *)a,
                       (const uint16_t *)b, c, d);
    return check(hipGetLastError(), "mfma probe launch") ? 1 : 0;
}

static unsigned probe_blocks(long long items)
{
    const long long blocks = (items + 255) / 256;
    return (unsigned)(blocks < 65536 ? blocks : 65536);
}

GENPC_API int genpc_grid_build_probe(int b, int n, const float *xyz, const int *noff, const int *moff, int cells_target, int cells_max,
                                     void *hdr, int *start, float *sorted, int *pos_of, int *orig_of, void *stream)
{
    using namespace genpc;
    if (!xyz || !hdr || !start || !sorted) { set_error("genpc_grid_build_probe: null buffer"); return -1; }
    if (moff) {
        RaggedTable t;
        int max_targets = 0;
        const char *err = nullptr;
        const int rc = ragged_table_fill(b, noff ? noff : moff, moff, t, &max_targets, &err);
        if (rc < 0) { set_error(err); return -1; }
        if (rc == 0 || max_targets == 0) return 0;
        return launch_cell_grid_build_ragged(t, max_targets, xyz, (CellGridHdr *)hdr, start, (float4 *)sorted, (hipStream_t)stream);
    }
    if (b < 1 || n < 1 || cells_target < 1 || cells_max < 1 || cells_max > kCellGridMaxCells || (long long)b * n > kRaggedMaxPoints) {
        set_error("genpc_grid_build_probe: b, n, cells_target >= 1 and 1 <= cells_max <= 15360 are required");
        return -1;
    }
    return launch_cell_grid_build(b, n, xyz, nullptr, (CellGridHdr *)hdr, start, (float4 *)sorted, pos_of, orig_of, cells_target, cells_max,
                                  (hipStream_t)stream);
}

GENPC_API int genpc_grid_size_probe(int nbox, int coarse, const float *mn, const float *mx, const int *cells_target, const int *cells_max,
                                    void *frames, void *stream)
{
    using namespace genpc;
    if (nbox < 0) return -1;
    if (nbox == 0) return 1;
    hipLaunchKernelGGL(grid_size_probe_kernel, dim3(probe_blocks(nbox)), dim3(256), 0, (hipStream_t)stream, nbox, coarse, mn, mx, cells_target,
                       cells_max, (GridFrame *)frames);
    return check(hipGetLastError(), "grid size probe launch") ? 1 : 0;
}

GENPC_API int genpc_grid_bound_probe(const void *hdr, int nq, const float *q, int n, const float *p, const float *mn, const float *mx,
                                     int gmax, int *qcell, int *pcell, float *qslack, float *gap1, float *gap4, float *bound, float *sq,
                                     float *slab, float *slab_bound, void *stream)
{
    using namespace genpc;
    if (nq < 1 || n < 1 || gmax < 1 || gmax > 1024 || (mn == nullptr) != (mx == nullptr)) {
        set_error("genpc_grid_bound_probe: nq, n >= 1, 1 <= gmax <= 1024 and both or neither of mn, mx are required");
        return -1;
    }
    const GridFrame *H = (const GridFrame *)hdr;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(grid_cell_probe_kernel, dim3(probe_blocks(3ll * (nq + n))), dim3(256), 0, st, H, nq, q, n, p, qcell, pcell, qslack);
    hipLaunchKernelGGL(grid_slab_probe_kernel, dim3(probe_blocks(3ll * nq * gmax)), dim3(256), 0, st, H, nq, q, gmax, mn, mx, slab, slab_bound);
    hipLaunchKernelGGL(grid_pair_probe_kernel, dim3(probe_blocks((long long)nq * n)), dim3(256), 0, st, H, nq, q, n, p, mn, mx, gap1, gap4, bound,
                       sq);
    return check(hipGetLastError(), "grid bound probe launch") ? 1 : 0;
}

GENPC_API int genpc_grid_range_probe(const void *hdr, int nq, const float *q, const float *radius, const int *clip, int *range, void *stream)
{
    using namespace genpc;
    if (nq < 0) return -1;
    if (nq == 0) return 1;
    hipLaunchKernelGGL(grid_range_probe_kernel, dim3(probe_blocks(3ll * nq)), dim3(256), 0, (hipStream_t)stream, (const GridFrame *)hdr, nq, q,
                       radius, clip, range);
    return check(hipGetLastError(), "grid range probe launch") ? 1 : 0;
}
