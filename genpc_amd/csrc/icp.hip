// icp.hip -- batched point-to-point ICP and the scale-search scoring of reg_xyz.py
//  for gfx950.
//
// The reference runs 11 + 1000 open3d ICP solves on the CPU, one candidate scale at
// a time, each followed by two chamfer_3DDist calls on ~1-5 k-point clouds with
// numpy <-> torch <-> GPU round trips (reg_xyz.py:60-96,146-173) -- launch- and
// transfer-bound.  Here K candidates that share the source and target clouds and
// differ only in their initial 4x4 transform are solved together: per ICP pass
//   icp_transform_kernel   p' = T_k p for all K candidates (T in double, p' fp32)
//   nn_forward_kernel      one batched NN launch, B = K (chamfer.hip)
//   icp_accum_kernel       Kabsch sums over the correspondences with d2 <= r^2
//                          (fp64 wave/block reduction, 17 atomics per block)
//   icp_update_kernel      one thread per candidate: fitness / rmse, open3d's
//                          convergence test, Horn's quaternion solve (4x4 Jacobi),
//                          T_k <- update T_k
// with no host synchronisation; converged candidates idle.  The 1000-candidate
// anisotropic scale search scores every candidate with ONE batched NN launch
// (B = 1000): its score (reg_xyz.py:77-83) depends on the scaled source only, not
// on the ICP result, so only the winner needs an ICP solve.
// Numerics follow oracle/genpc_oracle_geom.c (oracle_icp): same fp32 NN, sums in
// double; sums are reduced in a different order (1e-12 relative).
#include "nn.h"
#include "ragged_table.h"
#define GENPC_ICP_PLAN_HD GENPC_RAGGED_HD          // icp_plan() on the device too: icp_fused_ragged_kernel
#include "icp_ragged_plan.h"
#include "ragged_cand.h"
#include "cd_score.h"                              // kIBlock, and the score's sums in their one order
#include "../../include/genpc_hip.h"

#include <math.h>

extern "C" int genpc_nm_distance(int b, int n, const float *xyz, int m, const float *xyz2, float *result,
                                 int *result_i, void *stream);
extern "C" int genpc_chamfer_forward(int b, int n, const float *xyz1, int m, const float *xyz2, float *dist1,
                                     int *idx1, float *dist2, int *idx2, void *stream);

namespace genpc {

struct IcpState {
    double prev_fitness, prev_rmse;
    int done, iters;
};

// p' = T p: the product in double, rounded to fp32 (oracle: icp_evaluate)
__device__ __forceinline__ void icp_map_point(const double *m, const float *__restrict__ p, float &ox, float &oy, float &oz)
{
    const double x = p[0], y = p[1], z = p[2];
    ox = (float)(m[0] * x + m[1] * y + m[2] * z + m[3]);
    oy = (float)(m[4] * x + m[5] * y + m[6] * z + m[7]);
    oz = (float)(m[8] * x + m[9] * y + m[10] * z + m[11]);
}

__device__ __forceinline__ void icp_map_point(const double *m, float sx, float sy, float sz, float &ox, float &oy, float &oz)
{
    const float p[3] = {sx, sy, sz};
    icp_map_point(m, p, ox, oy, oz);
}

__global__ __launch_bounds__(kIBlock) void icp_transform_kernel(int ns, const float *__restrict__ source,
                                                                const double *__restrict__ T,
                                                                float *__restrict__ pts)
{
    const int c = blockIdx.y;
    const double *M = T + (size_t)c * 16;
    double m[12];
#pragma unroll
    for (int k = 0; k < 12; k++) m[k] = M[k];
    for (int j = blockIdx.x * kIBlock + threadIdx.x; j < ns; j += gridDim.x * kIBlock) {
        float *o = pts + ((size_t)c * ns + j) * 3;
        icp_map_point(m, source + (size_t)j * 3, o[0], o[1], o[2]);
    }
}

// out[c, j, :] = in[j, :] * scale[c, :]   (double product rounded to fp32); scale == nullptr: plain replicate
__global__ __launch_bounds__(kIBlock) void replicate_scale_kernel(int n, const float *__restrict__ in,
                                                                  const float *__restrict__ scale,
                                                                  float *__restrict__ out)
{
    const int c = blockIdx.y;
    double s[3] = {1.0, 1.0, 1.0};
    if (scale) {
        s[0] = scale[c * 3 + 0]; s[1] = scale[c * 3 + 1]; s[2] = scale[c * 3 + 2];
    }
    for (int j = blockIdx.x * kIBlock + threadIdx.x; j < n; j += gridDim.x * kIBlock) {
        float *o = out + ((size_t)c * n + j) * 3;
        if (scale) {
            o[0] = (float)((double)in[(size_t)j * 3 + 0] * s[0]);
            o[1] = (float)((double)in[(size_t)j * 3 + 1] * s[1]);
            o[2] = (float)((double)in[(size_t)j * 3 + 2] * s[2]);
        } else {
            o[0] = in[(size_t)j * 3 + 0]; o[1] = in[(size_t)j * 3 + 1]; o[2] = in[(size_t)j * 3 + 2];
        }
    }
}

// accum[c, 17]: n, sum p[3], sum q[3], sum p q^T [9], sum d2
__global__ __launch_bounds__(kIBlock) void icp_accum_kernel(int ns, const float *__restrict__ pts,
                                                            const float *__restrict__ target,
                                                            const float *__restrict__ d, const int *__restrict__ idx,
                                                            float md2, double *__restrict__ accum)
{
    __shared__ double red[17][kIBlock / kWave];
    const int c = blockIdx.y;
    double a[17];
#pragma unroll
    for (int k = 0; k < 17; k++) a[k] = 0.0;
    for (int j = blockIdx.x * kIBlock + threadIdx.x; j < ns; j += gridDim.x * kIBlock) {
        const float dj = d[(size_t)c * ns + j];
        if (!(dj <= md2)) continue;
        const float *p = pts + ((size_t)c * ns + j) * 3;
        const float *q = target + (size_t)idx[(size_t)c * ns + j] * 3;
        const double pp[3] = {p[0], p[1], p[2]}, qq[3] = {q[0], q[1], q[2]};
        a[0] += 1.0;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            a[1 + r] += pp[r];
            a[4 + r] += qq[r];
#pragma unroll
            for (int s = 0; s < 3; s++) a[7 + r * 3 + s] += pp[r] * qq[s];
        }
        a[16] += (double)dj;
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 17; k++) {
        double x = a[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, kWave);
        if (lane == 0) red[k][wave] = x;
    }
    __syncthreads();
    if (threadIdx.x < 17) {
        double x = 0.0;
#pragma unroll
        for (int w = 0; w < kIBlock / kWave; w++) x += red[threadIdx.x][w];
        atomicAdd(&accum[(size_t)c * 17 + threadIdx.x], x);
    }
}

// Cyclic Jacobi on the symmetric 4x4.  Converged when the off-diagonal mass is rounding noise RELATIVE to the matrix
// (an absolute threshold of 1e-300 is never met: a rotated-away element comes back as noise of size 1e-16 |A|, and all 30
// sweeps ran -- 35 us per ICP pass in one lane, fp64 divisions and square roots; now 5-7 sweeps).
// 1 / sqrt(x), x normal and positive: the hardware estimate and two Newton steps (relative error ~1e-16)
__device__ __forceinline__ double rsqrt_f64(double x)
{
    double y = __builtin_amdgcn_rsq(x);
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const double e = __builtin_fma(-x * y, y, 1.0);        // 1 - x y^2
        y = __builtin_fma(y * 0.5, e, y);
    }
    return y;
}

// (Every index below is a compile-time constant once the loops are unrolled: the matrices live in registers -- as arrays indexed by
// loop variables they sat in scratch memory, and the update was 12 us of one lane per pass.)
__device__ __forceinline__ void jacobi4(double (&A)[4][4], double (&V)[4][4])
{
    double norm2 = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            V[i][j] = (i == j) ? 1.0 : 0.0;
            norm2 += A[i][j] * A[i][j];
        }
    const double tiny2 = 1e-32 * norm2;          // an element below 1e-16 |A|: rounding noise of the rotations themselves
    for (int sweep = 0; sweep < 30; sweep++) {
        double off = 0.0;
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = i + 1; j < 4; j++) off += A[i][j] * A[i][j];
        if (!(off > tiny2)) break;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                if (!(A[p][q] * A[p][q] > tiny2)) continue;
                // the rotation that zeroes A[p][q]: with d = A[q][q] - A[p][p], b = 2 A[p][q], r = |(d, b)|:  cos 2phi = |d| / r,
                // sin 2phi = sgn(d) b / r, c = sqrt((1 + cos 2phi) / 2), s = sin 2phi / (2 c) -- the rotation of the textbook form
                // (theta = d / b, t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c) with two reciprocal
                // square roots instead of three divisions and two square roots (each a ~40-instruction dependent chain in fp64:
                // the update was 12 us of one lane per pass)
                const double d = A[q][q] - A[p][p], b = 2.0 * A[p][q];
                const double inv_r = rsqrt_f64(d * d + b * b);
                const double c2 = 0.5 + 0.5 * fabs(d) * inv_r;
                const double inv_c = rsqrt_f64(c2);
                const double c = c2 * inv_c, s = (d >= 0 ? 0.5 : -0.5) * b * inv_r * inv_c;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                A[p][q] = A[q][p] = 0.0;          // (what the rotation was chosen for)
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
}

// Horn's closed-form absolute orientation from the Kabsch sums
__device__ __forceinline__ void kabsch_from_sums(const double *sums, double *U)
{
    const double n = sums[0], inv_n = 1.0 / n;
    const double mp[3] = {sums[1] * inv_n, sums[2] * inv_n, sums[3] * inv_n};
    const double mq[3] = {sums[4] * inv_n, sums[5] * inv_n, sums[6] * inv_n};
    double S[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) S[a][b] = sums[7 + a * 3 + b] - n * mp[a] * mq[b];
    double N[4][4] = {
        {S[0][0] + S[1][1] + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0]},
        {S[1][2] - S[2][1], S[0][0] - S[1][1] - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2]},
        {S[2][0] - S[0][2], S[0][1] + S[1][0], -S[0][0] + S[1][1] - S[2][2], S[1][2] + S[2][1]},
        {S[0][1] - S[1][0], S[2][0] + S[0][2], S[1][2] + S[2][1], -S[0][0] - S[1][1] + S[2][2]}};
    double V[4][4];
    jacobi4(N, V);
    // the eigenvector of the largest eigenvalue (the first of equals)
    double lam = N[0][0], w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];
#pragma unroll
    for (int i = 1; i < 4; i++)
        if (N[i][i] > lam) {
            lam = N[i][i];
            w = V[0][i]; x = V[1][i]; y = V[2][i]; z = V[3][i];
        }
    const double inn = rsqrt_f64(w * w + x * x + y * y + z * z);
    w *= inn; x *= inn; y *= inn; z *= inn;
    const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)},
                            {2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)},
                            {2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)}};
#pragma unroll
    for (int a = 0; a < 3; a++) {
#pragma unroll
        for (int b = 0; b < 3; b++) U[a * 4 + b] = R[a][b];
        U[a * 4 + 3] = mq[a] - (R[a][0] * mp[0] + R[a][1] * mp[1] + R[a][2] * mp[2]);
    }
    U[12] = U[13] = U[14] = 0.0;
    U[15] = 1.0;
}

// One candidate, after the pass's sums: fitness / rmse, open3d's convergence test, the Kabsch step.  (Does not clear the sums.)
__device__ void icp_update_one(const double *A, double *Tc, IcpState &S, double *stats, int ns, int pass, int max_iter,
                               double rel_fitness, double rel_rmse)
{
    if (pass == 0) {
        S.done = 0;
        S.iters = 0;
    }
    if (S.done) return;
    const double n = A[0];
    const double fitness = n / ns, rmse = n > 0 ? sqrt(A[16] / n) : 0.0;
    if (pass > 0) {
        S.iters += 1;
        if (fabs(S.prev_fitness - fitness) < rel_fitness && fabs(S.prev_rmse - rmse) < rel_rmse) S.done = 1;
    }
    S.prev_fitness = fitness;
    S.prev_rmse = rmse;
    stats[0] = fitness;
    stats[1] = rmse;
    stats[2] = (double)S.iters;
    if (S.done) return;
    if (pass >= max_iter || n < 1.0) {
        S.done = 1;
        return;
    }
    double U[16], Tn[16];
    kabsch_from_sums(A, U);
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            double acc = 0.0;
#pragma unroll
            for (int q = 0; q < 4; q++) acc += U[a * 4 + q] * Tc[q * 4 + b];
            Tn[a * 4 + b] = acc;
        }
#pragma unroll
    for (int q = 0; q < 16; q++) Tc[q] = Tn[q];
}

__global__ void icp_update_kernel(int k, int ns, double *__restrict__ accum, double *__restrict__ T,
                                  IcpState *__restrict__ state, double *__restrict__ stats, int pass, int max_iter,
                                  double rel_fitness, double rel_rmse)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= k) return;
    double *A = accum + (size_t)c * 17;
    icp_update_one(A, T + (size_t)c * 16, state[c], stats + (size_t)c * 3, ns, pass, max_iter, rel_fitness, rel_rmse);
    for (int q = 0; q < 17; q++) A[q] = 0.0;
}

// scores[c] = mean sqrt(d1[c,:]) + w * mean sqrt(d2[c,:])   (reg_xyz.py:81-83,167-169)
__global__ __launch_bounds__(kIBlock) void cd_score_kernel(int n1, const float *__restrict__ d1, int n2,
                                                           const float *__restrict__ d2, float w,
                                                           float *__restrict__ scores)
{
    __shared__ double red[2][kIBlock / kWave];
    const int c = blockIdx.x;
    const double a = cd_score_thread_sum(n1, [&](int j) { return d1[(size_t)c * n1 + j]; });
    const double b = cd_score_thread_sum(n2, [&](int j) { return d2[(size_t)c * n2 + j]; });
    cd_score_reduce(a, b, n1, n2, w, &red[0][0], scores + c);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The whole solve of one candidate in ONE workgroup (round 6).  The five launches per pass above cost ~45 us per pass at the
// pipeline's sizes (3-5 k points a side: every kernel is a few microseconds of work behind a launch and a device-wide kernel
// boundary), 31 passes a solve, six solves a completed scan: ~8 ms of a 38 ms scan and 930 of its 2100 launches (with six scans
// in flight the device runs ~90 k kernels per second whatever the number of queues: the launches are the limit there).
//
// ICP uses a correspondence only when its squared distance is <= max_dist^2, so the nearest-neighbour search needs no more than
// the targets within max_dist of the query: the target cloud goes ONCE into a uniform grid in LDS (grid.h's frame, cell function
// and counting sort; cell >= 1.001 max_dist: a target within max_dist lies in the 27 cells around the query's), and a pass is,
// per wave and 64 queries at a time,
//   p' = T p (registers) -> the home cell's points -> three rounds (one plane of 9 neighbour cells each): the (query, cell) pairs
//   whose box can still hold a point nearer than the query's best so far (or than max_dist) go to a wave-private list in LDS and are
//   worked off one pair per lane (ds_min_u64 on distance bits << 32 | index: the smallest distance, the lowest index among equals,
//   which is the order of the exhaustive search) -> Kabsch sums of the inliers in double registers
// -- no workgroup barrier inside --, then a fixed-order reduction (lane tree, waves in order: the sums do not depend on timing,
// unlike the atomics above) and the update by one thread.  Distances: sqdist<FMA>, the arithmetic of the exhaustive search.
// A (query, cell) pair is left out by the Bound of grid.h alone: only when no point of the cell can tie or beat the limit in fp32.
// (kFT threads, kFWaves waves, kFItems pairs per wave and round, and what of the LDS is whose: icp_plan.h)
static_assert(kFWaves * kWave == kFT, "icp_plan.h counts waves of 64 lanes");
constexpr int kFAxis = 64;                   // cells per axis at most

// key of a candidate: distance bits << 32 | index << 16 | position in P -- the smallest distance, the lowest index among equals
template <int FMA>
__device__ __forceinline__ unsigned long long icp_key(const float4 v, unsigned pos, float px, float py, float pz)
{
    const float d = sqdist<FMA>(v.x - px, v.y - py, v.z - pz);
    return ((unsigned long long)__float_as_uint(d) << 32) | ((unsigned)__float_as_int(v.w) << 16) | pos;
}
// the points P[b, e) against one query, four at a time (four LDS reads in flight; the last group repeats the last point)
template <int FMA>
__device__ __forceinline__ unsigned long long icp_scan_cell(const float4 *__restrict__ P, unsigned b, unsigned e, float px, float py, float pz,
                                                            unsigned long long key)
{
    for (unsigned t = b; t < e; t += 4) {
        const unsigned l = e - 1;
        const unsigned t1 = t + 1 < l ? t + 1 : l, t2 = t + 2 < l ? t + 2 : l, t3 = t + 3 < l ? t + 3 : l;
        const float4 v0 = P[t], v1 = P[t1], v2 = P[t2], v3 = P[t3];
        unsigned long long k0 = icp_key<FMA>(v0, t, px, py, pz), k1 = icp_key<FMA>(v1, t1, px, py, pz);
        const unsigned long long k2 = icp_key<FMA>(v2, t2, px, py, pz), k3 = icp_key<FMA>(v3, t3, px, py, pz);
        k0 = k0 < k2 ? k0 : k2;
        k1 = k1 < k3 ? k1 : k3;
        k0 = k0 < k1 ? k0 : k1;
        key = k0 < key ? k0 : key;
    }
    return key;
}

#define ICP_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                             __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

// tools/icp_timeline.py builds a private copy with -DGENPC_ICP_TIMELINE: thread 0 of candidate 0 stamps the wall clock (100 MHz)
// at the start, after the grid, and per pass after the search, the reduction and the update.
#ifdef GENPC_ICP_TIMELINE
__device__ unsigned long long g_icp_tl[2 + 3 * 64];
#define ICP_STAMP(i) do { if (tid == 0 && cand == 0 && (i) < 2 + 3 * 64) g_icp_tl[i] = wall_clock64(); } while (0)
#else
#define ICP_STAMP(i) do { } while (0)
#endif

// The solve of candidate `cand` by the calling workgroup: init, out_T and stats are the call's arrays, indexed by cand; the clouds
// are the candidate's own.  The one statement of the arithmetic: icp_fused_kernel and icp_fused_ragged_kernel are this and nothing else.
template <int FMA>
__device__ __forceinline__ void icp_fused_solve(int cand, int ns, const float *__restrict__ source, int nt, const float *__restrict__ target,
                                                float md2, double max_dist, const double *__restrict__ init, int max_iter,
                                                double rel_fitness, double rel_rmse, int cells_cap, double *__restrict__ out_T,
                                                double *__restrict__ stats)
{
    extern __shared__ __align__(16) unsigned char icp_lds[];
    __shared__ GridFrame F;
    __shared__ float s_mx[3];                  // the cloud's maximum (its minimum is F.lo): the outer walls of the border cells
    __shared__ IcpState s_state;
    __shared__ float s_red[6 * kFWaves];       // the box reduction's, then the scan's
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int ntp = (nt + 3) & ~3;
    float4 *P = (float4 *)icp_lds;                                   // [ntp] targets in cell order: x, y, z, index
    unsigned *cend = (unsigned *)(P + ntp);                          // [cells_cap] end of each cell's run in P
    float4 *Qw = (float4 *)(cend + cells_cap) + wave * kWave;        // per wave: the 64 queries of the batch
    unsigned long long *keys = (unsigned long long *)((float4 *)(cend + cells_cap) + kFT) + wave * kWave;      // per wave: their best so far
    unsigned *items = (unsigned *)((unsigned long long *)((float4 *)(cend + cells_cap) + kFT) + kFT) + wave * kFItems;     // per wave: query | cell << 6
    double *red = (double *)((unsigned *)((unsigned long long *)((float4 *)(cend + cells_cap) + kFT) + kFT) + kFWaves * kFItems);   // [17][waves]
    double *s_T = red + 17 * kFWaves;                                // [16]
    double *s_sums = s_T + 16;                                       // [17]

    ICP_STAMP(0);
    // ---- the grid of the target cloud
    {
        float mn[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, mx[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
        for (int t = tid; t < nt; t += kFT)
            for (int a = 0; a < 3; a++) {
                const float v = target[(size_t)t * 3 + a];
                mn[a] = fminf(mn[a], v);
                mx[a] = fmaxf(mx[a], v);
            }
        grid_block_box<kFT>(mn, mx, s_red);
        if (tid == 0) {
            // The sizing is this kernel's own.  The 27 cells: for |p - q| <= max_dist (1 + 4u) on an axis -- what an fp32 distance of
            // at most md2 allows -- the exact cell coordinates differ by at most (1 + 5u) / 1.001 < 0.99901; a computed one,
            // fl(fl(p - lo) * inv), errs by at most 3u |t| (1 + 2u), and |t| <= 66 wherever it matters (the cell function is
            // monotone and clamped: beyond the grid's ends every floor is the same cell or its sentinel): 2 * 198u < 2.4e-5.  The
            // computed coordinates differ by less than 1, their floors by at most one.
            float mag = 0.0f, ext[3];
            for (int a = 0; a < 3; a++) {
                ext[a] = mx[a] - mn[a];
                mag = fmaxf(mag, fmaxf(fabsf(mn[a]), fabsf(mx[a])));
            }
            float h = (float)(max_dist * 1.001);
            const bool one = !(h > 1e-30f) || !(h < 1e30f) || !(mag < 1e30f);      // one cell: every target is a neighbour of every query
            int g[3] = {1, 1, 1};
            while (!one) {
                long long cells = 1;
                for (int a = 0; a < 3; a++) {
                    const float q = ext[a] / h;
                    g[a] = q >= (float)(kFAxis - 1) ? kFAxis : (int)q + 1;
                    cells *= g[a];
                }
                if (cells <= cells_cap) break;
                h *= 1.25f;
            }
            grid_frame(mn, g, one ? 1.0f : h, F);
            for (int a = 0; a < 3; a++) s_mx[a] = mx[a];
            for (int q = 0; q < 16; q++) s_T[q] = init[(size_t)cand * 16 + q];
        }
    }
    __syncthreads();
    const int c0 = F.g[0], c1 = F.g[1], c2 = F.g[2];
    const float inv = F.inv, h = F.h;
    auto cell_of = [&](float x, float y, float z) {
        return (grid_cell1(z, F.lo[2], inv, c2) * c1 + grid_cell1(y, F.lo[1], inv, c1)) * c0 + grid_cell1(x, F.lo[0], inv, c0);
    };
    const int cells = c0 * c1 * c2;
    for (int q = tid; q < cells; q += kFT) cend[q] = 0;
    __syncthreads();
    for (int t = tid; t < nt; t += kFT)
        atomicAdd(&cend[cell_of(target[(size_t)t * 3 + 0], target[(size_t)t * 3 + 1], target[(size_t)t * 3 + 2])], 1u);
    __syncthreads();
    grid_scan_counts<kFT>((int *)cend, cells, 0, (int *)s_red);
    for (int t = tid; t < nt; t += kFT) {
        const float x = target[(size_t)t * 3 + 0], y = target[(size_t)t * 3 + 1], z = target[(size_t)t * 3 + 2];
        const unsigned pos = atomicAdd(&cend[cell_of(x, y, z)], 1u);        // afterwards cend[c] is the END of cell c's run
        P[pos] = make_float4(x, y, z, __int_as_float(t));
    }
    __syncthreads();

    ICP_STAMP(1);
    const unsigned long long kNone = ((unsigned long long)0x7f800000u << 32) | 0xffffffffu;      // (+inf, nothing)
    for (int pass = 0; pass <= max_iter; pass++) {
        double m[12];
#pragma unroll
        for (int q = 0; q < 12; q++) m[q] = s_T[q];
        double acc[17];
#pragma unroll
        for (int q = 0; q < 17; q++) acc[q] = 0.0;
        float sx = 0.0f, sy = 0.0f, sz = 0.0f;          // the batch's source point (loaded one batch ahead)
        if (wave * kWave + lane < ns) {
            const float *sp = source + (size_t)(wave * kWave + lane) * 3;
            sx = sp[0]; sy = sp[1]; sz = sp[2];
        }
        for (int b0 = wave * kWave; b0 < ns; b0 += kFT) {
            const int j = b0 + lane;
            const bool valid = j < ns;
            float px = 0.0f, py = 0.0f, pz = 0.0f;
            int cx = -1, cy = -1, cz = -1;
            unsigned long long key = kNone;
            if (valid) icp_map_point(m, sx, sy, sz, px, py, pz);
            if (j + kFT < ns) {
                const float *sp = source + (size_t)(j + kFT) * 3;
                sx = sp[0]; sy = sp[1]; sz = sp[2];
            }
            if (valid) {
                // cell coordinates by grid_cell1's two operations, but -1 and c for "before" / "beyond" the grid (NaN: -1)
                cx = (int)fminf(fmaxf(floorf(__fmul_rn(__fsub_rn(px, F.lo[0]), inv)), -1.0f), (float)c0);
                cy = (int)fminf(fmaxf(floorf(__fmul_rn(__fsub_rn(py, F.lo[1]), inv)), -1.0f), (float)c1);
                cz = (int)fminf(fmaxf(floorf(__fmul_rn(__fsub_rn(pz, F.lo[2]), inv)), -1.0f), (float)c2);
                if (cx >= 0 && cx < c0 && cy >= 0 && cy < c1 && cz >= 0 && cz < c2) {
                    const int cell = (cz * c1 + cy) * c0 + cx;
                    key = icp_scan_cell<FMA>(P, cell ? cend[cell - 1] : 0u, cend[cell], px, py, pz, key);
                }
            }
            Qw[lane] = make_float4(px, py, pz, 0.0f);
            keys[lane] = key;
            // the neighbour cells that can still hold a point that ties or beats the best so far (or max_dist)
            unsigned mask = 0;
            if (valid) {
                const float lim = fminf(__uint_as_float((unsigned)(key >> 32)), md2);
                // (queries lie outside the box: the border cells end at the cloud's own minimum, F.lo, and maximum)
                const float slx = grid_slack(F.slack[0], px), sly = grid_slack(F.slack[1], py), slz = grid_slack(F.slack[2], pz);
                float gx[3], gy[3], gz[3];
#pragma unroll
                for (int o = 0; o < 3; o++) {
                    const int ix = cx + o - 1, iy = cy + o - 1, iz = cz + o - 1;
                    gx[o] = ix >= 0 && ix < c0 ? grid_gap(ix, 1, c0, F.lo[0], h, px, slx, F.lo[0], s_mx[0]) : __builtin_inff();
                    gy[o] = iy >= 0 && iy < c1 ? grid_gap(iy, 1, c1, F.lo[1], h, py, sly, F.lo[1], s_mx[1]) : __builtin_inff();
                    gz[o] = iz >= 0 && iz < c2 ? grid_gap(iz, 1, c2, F.lo[2], h, pz, slz, F.lo[2], s_mx[2]) : __builtin_inff();
                }
#pragma unroll
                for (int pl = 0; pl < 3; pl++) {
                    // the plane's nine runs first (18 LDS reads in flight), then the tests
                    unsigned rb[9], re[9];
                    const int nz = min(max(cz + pl - 1, 0), c2 - 1);
#pragma unroll
                    for (int k = 0; k < 9; k++) {
                        const int nx = min(max(cx + k % 3 - 1, 0), c0 - 1), ny = min(max(cy + k / 3 - 1, 0), c1 - 1);
                        const int cell = (nz * c1 + ny) * c0 + nx;
                        re[k] = cend[cell];
                        rb[k] = cend[cell > 0 ? cell - 1 : 0];
                        if (cell == 0) rb[k] = 0u;
                    }
#pragma unroll
                    for (int k = 0; k < 9; k++) {
                        if (pl == 1 && k == 4) continue;
                        const float g = __fmaf_rn(gx[k % 3], gx[k % 3], __fmaf_rn(gy[k / 3], gy[k / 3], __fmul_rn(gz[pl], gz[pl])));   // (+inf: outside the grid)
                        if (!(g * kGridShrink > lim) && rb[k] != re[k]) mask |= 1u << (pl * 9 + k);       // (kept at equality: dj <= md2 counts)
                    }
                }
            }
            int cnt = __popc(mask);
            ICP_WAVE_SYNC();
            for (;;) {
                const int incl = wave_scan_incl(cnt);
                const int total = __builtin_amdgcn_readlane(incl, kWave - 1);
                if (total == 0) break;
                int w = incl - cnt;
                while (mask && w < kFItems) {
                    const int sl = __ffs(mask) - 1;
                    mask &= mask - 1;
                    const int cell = ((cz + sl / 9 - 1) * c1 + cy + (sl / 3) % 3 - 1) * c0 + cx + sl % 3 - 1;
                    items[w++] = (unsigned)lane | ((unsigned)cell << 6);
                }
                cnt = __popc(mask);
                ICP_WAVE_SYNC();
                const int todo = total < kFItems ? total : kFItems;
                for (int i = lane; i < todo; i += kWave) {
                    const unsigned it = items[i];
                    const int q = it & 63, cell = it >> 6;
                    const float4 Q = Qw[q];
                    const unsigned long long k = icp_scan_cell<FMA>(P, cell ? cend[cell - 1] : 0u, cend[cell], Q.x, Q.y, Q.z, kNone);
                    atomicMin(&keys[q], k);
                }
                ICP_WAVE_SYNC();
            }
            key = keys[lane];
            const float dj = __uint_as_float((unsigned)(key >> 32));
            if (valid && dj <= md2) {
                const float4 qv = P[(unsigned)key & 0xffffu];
                const double pp[3] = {px, py, pz}, qq[3] = {qv.x, qv.y, qv.z};
                acc[0] += 1.0;
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    acc[1 + a] += pp[a];
                    acc[4 + a] += qq[a];
#pragma unroll
                    for (int b = 0; b < 3; b++) acc[7 + a * 3 + b] += pp[a] * qq[b];
                }
                acc[16] += (double)dj;
            }
            __builtin_amdgcn_wave_barrier();          // (the next batch rewrites Qw / keys)
        }
        ICP_STAMP(2 + pass * 3);
        // fixed-order reduction: the lanes on the DPP network, then the waves in order
#pragma unroll
        for (int q = 0; q < 17; q++) {
            const double x = wave_sum63(acc[q]);
            if (lane == kWave - 1) red[q * kFWaves + wave] = x;
        }
        __syncthreads();
        if (wave == 0) {
            if (lane < 17) {
                double x = 0.0;
#pragma unroll
                for (int w = 0; w < kFWaves; w++) x += red[lane * kFWaves + w];
                s_sums[lane] = x;
            }
            ICP_WAVE_SYNC();
            ICP_STAMP(3 + pass * 3);
            if (lane == 0) icp_update_one(s_sums, s_T, s_state, stats + (size_t)cand * 3, ns, pass, max_iter, rel_fitness, rel_rmse);
        }
        __syncthreads();
        ICP_STAMP(4 + pass * 3);
        if (s_state.done) break;
    }
    if (tid < 16) out_T[(size_t)cand * 16 + tid] = s_T[tid];
}

template <int FMA>
__global__ __launch_bounds__(kFT) void icp_fused_kernel(int ns, const float *__restrict__ source, int nt, const float *__restrict__ target,
                                                        float md2, double max_dist, const double *__restrict__ init, int max_iter,
                                                        double rel_fitness, double rel_rmse, int cells_cap, double *__restrict__ out_T,
                                                        double *__restrict__ stats)
{
    icp_fused_solve<FMA>(blockIdx.x, ns, source, nt, target, md2, max_dist, init, max_iter, rel_fitness, rel_rmse, cells_cap, out_T, stats);
}

// genpc_icp_batch_ragged's one launch: workgroup blockIdx.x solves candidate blockIdx.x of the call.  Its pair -- the largest j
// with koff[j] <= candidate, ragged_cand.h's uniform search of the table in the kernel arguments (scalar loads) -- gives it its own
// ns, nt, clouds and, through icp_plan(nt), its own cell budget, by which icp_fused_solve carves the LDS (ntp, cells_cap): the
// launch's dynamic LDS is the largest of the pairs' (icp_ragged_plan.h).  A candidate of a multi-launch pair leaves at once.
struct IcpRaggedArgs {
    RaggedCandTable t;                         // (first: the layout of the kernel arguments)
    const float *source, *target;              // packed
    const double *init;                        // [K,16]
    double *out_T, *stats;                     // [K,16], [K,3]
    double max_dist, rel_fitness, rel_rmse;
    float md2;
    int max_iter;
};
static_assert(sizeof(IcpRaggedArgs) <= 4096, "the pair table must fit the kernel arguments");
static_assert(kIcpRaggedMaxPairs == kRaggedCandMaxPairs && kIcpRaggedMaxPoints == kRaggedCandMaxPoints &&
              kIcpRaggedMaxCandidates == kRaggedCandMaxCandidates, "ragged_cand.h checks and carries the table");

template <int FMA>
__global__ __launch_bounds__(kFT) void icp_fused_ragged_kernel(IcpRaggedArgs a)
{
    const int cand = blockIdx.x, pair = ragged_cand_pair_of(a.t, cand);
    const int s0 = a.t.soff[pair], t0 = a.t.toff[pair];
    const int ns = a.t.soff[pair + 1] - s0, nt = a.t.toff[pair + 1] - t0;
    const IcpPlan plan = icp_plan(nt);
    if (!plan.one_workgroup) return;                  // (uniform: the whole workgroup leaves)
    icp_fused_solve<FMA>(cand, ns, a.source + (size_t)s0 * 3, nt, a.target + (size_t)t0 * 3, a.md2, a.max_dist, a.init, a.max_iter,
                         a.rel_fitness, a.rel_rmse, plan.cells, a.out_T, a.stats);
}

static int gx(int n)          // (not pose_plan.h's lin_grid: the same block of 256, but at most 64 blocks per row where that one allows 1024)
{
    int g = ceil_div(n, kIBlock);
    return g > 64 ? 64 : (g < 1 ? 1 : g);
}

}  // namespace genpc

GENPC_API int genpc_icp_batch(int k, int ns, const float *source, int nt, const float *target, double max_dist,
                              const double *init, int max_iter, double rel_fitness, double rel_rmse, double *out_T,
                              double *stats, void *stream)
{
    using namespace genpc;
    if (k <= 0 || ns <= 0 || nt <= 0 || max_iter < 0) return -1;
    hipStream_t st = (hipStream_t)stream;
    // the one-workgroup solve (one launch) when the target cloud and its grid fit a compute unit's LDS (icp_plan.h)
    const IcpPlan plan = icp_plan(nt);
    if (plan.one_workgroup) {
        const size_t lds = (size_t)plan.lds_bytes;
        const int fma = arith_mode() != 0 ? 1 : 0;
        static size_t set_bytes[2] = {0, 0};
        if (lds > set_bytes[fma]) {
            const hipError_t e = fma ? hipFuncSetAttribute((const void *)icp_fused_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)
                                     : hipFuncSetAttribute((const void *)icp_fused_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (!check(e, "hipFuncSetAttribute(icp_fused_kernel)")) return 0;
            set_bytes[fma] = lds;
        }
        const float md2f = (float)(max_dist * max_dist);
        if (fma)
            hipLaunchKernelGGL((icp_fused_kernel<1>), dim3(k), dim3(kFT), lds, st, ns, source, nt, target, md2f, max_dist, init, max_iter,
                               rel_fitness, rel_rmse, plan.cells, out_T, stats);
        else
            hipLaunchKernelGGL((icp_fused_kernel<0>), dim3(k), dim3(kFT), lds, st, ns, source, nt, target, md2f, max_dist, init, max_iter,
                               rel_fitness, rel_rmse, plan.cells, out_T, stats);
        return check(hipGetLastError(), "icp (one workgroup) launch") ? 1 : 0;
    }
    double *accum; IcpState *state; float *pts, *tgt, *d; int *idx;
    WsLayout L;
    L.add(accum, (size_t)k * 17);
    L.add(state, k);
    L.add(pts, (size_t)k * ns * 3);
    L.add(tgt, (size_t)k * nt * 3);          // the target once per candidate (k > 1)
    L.add(d, (size_t)k * ns);
    L.add(idx, (size_t)k * ns);
    if (!ws_alloc(L, kWsIcp, st)) return 0;
    if (!check(hipMemsetAsync(accum, 0, (size_t)k * 17 * 8, st), "hipMemsetAsync(icp accum)")) return 0;
    if (!check(hipMemcpyAsync(out_T, init, (size_t)k * 16 * 8, hipMemcpyDeviceToDevice, st), "copy init")) return 0;
    const float *tq = target;
    if (k > 1) {
        hipLaunchKernelGGL(replicate_scale_kernel, dim3(gx(nt), k), dim3(kIBlock), 0, st, nt, target,
                           (const float *)nullptr, tgt);
        tq = tgt;
    }
    // the target does not move: its duplicate mask (nn_dedupe.hip) is made once for all passes
    // (one row: the k candidates share the target)
    unsigned *dup_t = (unsigned *)workspace(kWsIcpDupMasks, nn_dedupe_mask_words(1, nt) * sizeof(unsigned), st);
    if (!dup_t) return 0;
    {
        const float *dp[2] = {target, nullptr};
        const int dn[2] = {nt, 0};
        unsigned *dm[2] = {dup_t, nullptr};
        if (!launch_nn_dedupe(1, 1, dp, dn, dm, nullptr, st)) return 0;
    }
    const float md2 = (float)(max_dist * max_dist);
    for (int pass = 0; pass <= max_iter; pass++) {
        hipLaunchKernelGGL(icp_transform_kernel, dim3(gx(ns), k), dim3(kIBlock), 0, st, ns, source,
                           (const double *)out_T, pts);
        if (nn_forward(k, 1, pts, ns, tq, nt, d, idx, nullptr, 0, nullptr, 0, nullptr, nullptr, st, __builtin_inff(), dup_t, nullptr, 1) != 1)
            return 0;
        hipLaunchKernelGGL(icp_accum_kernel, dim3(gx(ns), k), dim3(kIBlock), 0, st, ns, (const float *)pts, target,
                           (const float *)d, (const int *)idx, md2, accum);
        hipLaunchKernelGGL(icp_update_kernel, dim3(ceil_div(k, 64)), dim3(64), 0, st, k, ns, accum, out_T, state, stats,
                           pass, max_iter, rel_fitness, rel_rmse);
    }
    return check(hipGetLastError(), "icp launch") ? 1 : 0;
}

GENPC_API int genpc_icp_plan(int nt, int out[3])
{
    if (!out) return -1;
    const genpc::IcpPlan p = genpc::icp_plan(nt);
    out[0] = p.one_workgroup;
    out[1] = p.cells;
    out[2] = p.lds_bytes;
    return 1;
}

GENPC_API int genpc_icp_batch_ragged(int c, const int *soff, const int *toff, const int *koff, const float *source, const float *target,
                                     double max_dist, const double *init, int max_iter, double rel_fitness, double rel_rmse,
                                     double *out_T, double *stats, void *stream)
{
    using namespace genpc;
    const char *fn = "genpc_icp_batch_ragged";
    // every refusal is decided here, before anything touches a device: ragged_cand.h's about the table, and a negative number
    // of iterations, which ranks behind a negative number of pairs alone
    if (c >= 0 && max_iter < 0) return ragged_refuse(fn, "negative number of iterations");
    const char *what = nullptr;
    char buf[96];
    const int work = ragged_cand_check(c, soff, toff, koff, &what, buf);
    if (work <= 0) return work < 0 ? ragged_refuse(fn, what) : 1;
    const int k = koff[c];
    if (!source || !target || !init || !out_T || !stats) return ragged_refuse(fn, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    const IcpRaggedPlan plan = icp_ragged_plan(c, toff);
    if (plan.fused_pairs) {
        const size_t lds = (size_t)plan.lds_bytes;
        const int fma = arith_mode() != 0 ? 1 : 0;
        static size_t set_bytes[2] = {0, 0};
        if (lds > set_bytes[fma]) {
            const hipError_t e = fma ? hipFuncSetAttribute((const void *)icp_fused_ragged_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)
                                     : hipFuncSetAttribute((const void *)icp_fused_ragged_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (!check(e, "hipFuncSetAttribute(icp_fused_ragged_kernel)")) return 0;
            set_bytes[fma] = lds;
        }
        IcpRaggedArgs a{};
        ragged_cand_fill(a.t, c, soff, toff, koff);
        a.source = source; a.target = target; a.init = init; a.out_T = out_T; a.stats = stats;
        a.max_dist = max_dist; a.rel_fitness = rel_fitness; a.rel_rmse = rel_rmse;
        a.md2 = (float)(max_dist * max_dist);
        a.max_iter = max_iter;
        // one workgroup per candidate of the call; those of a multi-launch pair leave at once
        if (fma) hipLaunchKernelGGL((icp_fused_ragged_kernel<1>), dim3(k), dim3(kFT), lds, st, a);
        else hipLaunchKernelGGL((icp_fused_ragged_kernel<0>), dim3(k), dim3(kFT), lds, st, a);
        if (!check(hipGetLastError(), "icp (ragged, one workgroup) launch")) return 0;
    }
    if (plan.loop_pairs) {
        for (int j = 0; j < c; j++) {
            const int kj = koff[j + 1] - koff[j], nt = toff[j + 1] - toff[j];
            if (kj == 0 || icp_plan(nt).one_workgroup) continue;
            const int rc = genpc_icp_batch(kj, soff[j + 1] - soff[j], source + (size_t)soff[j] * 3, nt, target + (size_t)toff[j] * 3, max_dist,
                                           init + (size_t)koff[j] * 16, max_iter, rel_fitness, rel_rmse, out_T + (size_t)koff[j] * 16,
                                           stats + (size_t)koff[j] * 3, stream);
            if (rc != 1) return rc < 0 ? 0 : rc;
        }
    }
    return 1;
}

GENPC_API int genpc_icp_ragged_plan(int c, const int *toff, int out[3])
{
    using namespace genpc;
    const char *fn = "genpc_icp_ragged_plan";
    if (!out) return ragged_refuse(fn, "null pointer");
    out[0] = out[1] = out[2] = 0;
    const char *what = nullptr;
    const int some = ragged_cand_count(c, &what);
    if (some <= 0) return some < 0 ? ragged_refuse(fn, what) : 1;
    if (!toff) return ragged_refuse(fn, "null offset table");
    if ((what = ragged_offsets_fault(c, toff))) return ragged_refuse(fn, what);
    const IcpRaggedPlan p = icp_ragged_plan(c, toff);
    out[0] = p.fused_pairs;
    out[1] = p.loop_pairs;
    out[2] = p.lds_bytes;
    return 1;
}

#ifdef GENPC_ICP_TIMELINE
extern "C" __attribute__((visibility("default"))) int genpc_icp_timeline_read(unsigned long long *out)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(genpc::g_icp_tl), sizeof(unsigned long long) * (2 + 3 * 64)) == hipSuccess ? 1 : 0;
}
#endif

GENPC_API int genpc_scale_search_scores(int k, int ns, const float *source, int nt, const float *target,
                                        const float *scales, float cd_inv_weight, float *scores, void *stream)
{
    using namespace genpc;
    if (k <= 0 || ns <= 0 || nt <= 0) return -1;
    hipStream_t st = (hipStream_t)stream;
    float *src, *tgt, *d1, *d2; int *i1, *i2;
    WsLayout L;
    L.add(src, (size_t)k * ns * 3);
    L.add(tgt, (size_t)k * nt * 3);
    L.add(d1, (size_t)k * ns);
    L.add(i1, (size_t)k * ns);
    L.add(d2, (size_t)k * nt);
    L.add(i2, (size_t)k * nt);
    if (!ws_alloc(L, kWsScaleSearch, st)) return 0;
    hipLaunchKernelGGL(replicate_scale_kernel, dim3(gx(ns), k), dim3(kIBlock), 0, st, ns, source, scales, src);
    hipLaunchKernelGGL(replicate_scale_kernel, dim3(gx(nt), k), dim3(kIBlock), 0, st, nt, target,
                       (const float *)nullptr, tgt);
    // every candidate is a scaled copy of the one source against a copy of the one target: equal points stay equal under
    // any scale, so ONE row of duplicate marks per cloud (nn_dedupe.hip) serves all k candidates
    const size_t w_s = (nn_dedupe_mask_words(1, ns) + 63) & ~(size_t)63;
    unsigned *dup_s = (unsigned *)workspace(kWsIcpDupMasks, (w_s + nn_dedupe_mask_words(1, nt)) * sizeof(unsigned), st);
    if (!dup_s) return 0;
    unsigned *dup_t = dup_s + w_s;
    {
        const float *dp[2] = {target, source};
        const int dn[2] = {nt, ns};
        unsigned *dm[2] = {dup_t, dup_s};
        if (!launch_nn_dedupe(1, 2, dp, dn, dm, nullptr, st)) return 0;
    }
    if (nn_forward(k, 2, src, ns, tgt, nt, d1, i1, tgt, nt, src, ns, d2, i2, st, __builtin_inff(), dup_t, dup_s, 1) != 1) return 0;
    hipLaunchKernelGGL(cd_score_kernel, dim3(k), dim3(kIBlock), 0, st, ns, (const float *)d1, nt, (const float *)d2,
                       cd_inv_weight, scores);
    return check(hipGetLastError(), "scale_search_scores launch") ? 1 : 0;
}
