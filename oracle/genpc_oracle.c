/*
 * genpc_oracle.c -- CPU restatement of GenPC's geometric hot path.
 *
 * THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Only tests/, bench.py's
 * cpu_baseline leg and __graft_entry__.smoke() may load it, and only as the
 * checker.  The product path (genpc_amd/) never links, imports or calls it.
 *
 * Parity status: pinned to the reference's own kernel text.  oracle/ref_build.py
 * compiles the kernels of chamfer3D.cu and emd_cuda.cu, unmodified, for the CPU
 * (ref_simt.h, ref_driver.cpp -> oracle/_ref/), and tests/test_oracle_vs_reference.py
 * compares every function below with them bit for bit, in both arithmetic modes
 * (mode 1 = the contraction LLVM chooses; nvcc's is unverifiable).  Also pinned against:
 *   - the survey-time values in BASELINE.md section 2 (tests/test_oracle_golden.py)
 *   - an independent numpy restatement (tests/test_oracle_numpy.py)
 *   - float64 brute force / analytic gradients / exact-LAP bounds (properties)
 *
 * Every function cites the reference file:line it follows (paths relative to
 * the reference checkout).  Plain C11, no dependencies; OpenMP is used only to
 * spread independent queries / batch elements over host cores.
 *
 * Arithmetic modes (argument `fma_mode`):
 *   0  C semantics of the source text with NO floating-point contraction:
 *        d = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz))
 *   1  the contraction LLVM's DAG combiner applies to that expression under
 *      -ffp-contract=fast / nvcc -fmad=true (nvcc's default, hence what the
 *      shipped reference binary is expected to execute; unverifiable here):
 *        d = fma(dz, dz, fma(dx, dx, fl(dy*dy)))
 * Build with -ffp-contract=off so that mode 0 really is mode 0.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#define ORACLE_API __attribute__((visibility("default")))

static inline float sqdist(float dx, float dy, float dz, int fma_mode)
{
    if (fma_mode) {
        float t = dy * dy;
        t = fmaf(dx, dx, t);
        return fmaf(dz, dz, t);
    }
    float a = dx * dx;
    float b = dy * dy;
    float c = dz * dz;
    float s = a + b;
    return s + c;
}

ORACLE_API int oracle_num_threads(void)
{
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}

ORACLE_API void oracle_set_num_threads(int t)
{
#ifdef _OPENMP
    if (t > 0) omp_set_num_threads(t);
#else
    (void)t;
#endif
}

/* ------------------------------------------------------------------------
 * Chamfer forward, one direction.
 * Follows loss_functions/Chamfer3D/chamfer3D.cu:12-134 (NmDistanceKernel):
 *   dx = xyz2[k] - xyz[j] (target minus query, :32-34), d = x2*x2+y2*y2+z2*z2
 *   (:35); targets are scanned in tiles of 512 (:13,15-16); inside a tile the
 *   first target initialises `best` unconditionally and later ones replace it
 *   on a strict '<' (:36,46,56,66,119: 'k==0 || d<best'), so the lowest index
 *   wins ties; a tile's (best, best_i) replaces the running result on
 *   'k2==0 || result>best' (:126), which keeps the earlier tile on ties.
 *   For finite input the tiling does not change the answer.  For non-finite
 *   input it does, and the restatement keeps it: a NaN distance at the FIRST
 *   target of a tile makes that tile's best NaN (every later 'd<best' is
 *   false), and 'result>NaN' is false, so the whole tile is dropped -- unless
 *   it is tile 0, whose NaN becomes the result and is never replaced
 *   ('NaN>best' is false).  A NaN distance elsewhere in a tile only drops
 *   that one target.  The 4-way unrolling (:29-115) does not change the order
 *   of the comparisons and is not restated.
 *   m == 0 leaves result untouched (the k2 loop body never runs).
 * ---------------------------------------------------------------------- */
#define NM_TILE 512   /* chamfer3D.cu:13 `const int batch=512` */
ORACLE_API void oracle_nm_distance(int b, int n, const float *xyz, int m,
                                   const float *xyz2, float *result,
                                   int *result_i, int fma_mode)
{
    if (m <= 0) return;
    for (int i = 0; i < b; i++) {
        const float *q = xyz + (size_t)i * n * 3;
        const float *t = xyz2 + (size_t)i * m * 3;
#pragma omp parallel for schedule(static)
        for (int j = 0; j < n; j++) {
            float x1 = q[j * 3 + 0], y1 = q[j * 3 + 1], z1 = q[j * 3 + 2];
            float res = 0;
            int res_i = 0;
            for (int k2 = 0; k2 < m; k2 += NM_TILE) {
                int end_k = (m < k2 + NM_TILE ? m : k2 + NM_TILE) - k2;
                float best = 0;
                int best_i = 0;
                for (int k = 0; k < end_k; k++) {
                    float x2 = t[(k2 + k) * 3 + 0] - x1;
                    float y2 = t[(k2 + k) * 3 + 1] - y1;
                    float z2 = t[(k2 + k) * 3 + 2] - z1;
                    float d = sqdist(x2, y2, z2, fma_mode);
                    if (k == 0 || d < best) {
                        best = d;
                        best_i = k + k2;
                    }
                }
                if (k2 == 0 || res > best) {
                    res = best;
                    res_i = best_i;
                }
            }
            result[(size_t)i * n + j] = res;
            result_i[(size_t)i * n + j] = res_i;
        }
    }
}

/* chamfer_cuda_forward, chamfer3D.cu:136-154: two launches, A->B then B->A. */
ORACLE_API int oracle_chamfer_forward(int b, int n, const float *xyz1, int m,
                                      const float *xyz2, float *dist1,
                                      int *idx1, float *dist2, int *idx2,
                                      int fma_mode)
{
    oracle_nm_distance(b, n, xyz1, m, xyz2, dist1, idx1, fma_mode);
    oracle_nm_distance(b, m, xyz2, n, xyz1, dist2, idx2, fma_mode);
    return 1;
}

/* ------------------------------------------------------------------------
 * Chamfer backward.
 * Follows chamfer3D.cu:155-174 (NmDistanceGradKernel) and :176-195: both
 * directions accumulate into the two caller-zeroed buffers.  The reference
 * uses atomicAdd, so its summation order is unspecified; this restatement
 * accumulates sequentially (direction 1 ascending j, then direction 2
 * ascending k).  Compare with a relative tolerance.
 * ---------------------------------------------------------------------- */
static void nm_distance_grad(int b, int n, const float *xyz1, int m,
                             const float *xyz2, const float *grad_dist1,
                             const int *idx1, float *grad_xyz1,
                             float *grad_xyz2)
{
    for (int i = 0; i < b; i++) {
        for (int j = 0; j < n; j++) {
            float x1 = xyz1[((size_t)i * n + j) * 3 + 0];
            float y1 = xyz1[((size_t)i * n + j) * 3 + 1];
            float z1 = xyz1[((size_t)i * n + j) * 3 + 2];
            int j2 = idx1[(size_t)i * n + j];
            float x2 = xyz2[((size_t)i * m + j2) * 3 + 0];
            float y2 = xyz2[((size_t)i * m + j2) * 3 + 1];
            float z2 = xyz2[((size_t)i * m + j2) * 3 + 2];
            float g = grad_dist1[(size_t)i * n + j] * 2;
            float gx = g * (x1 - x2), gy = g * (y1 - y2), gz = g * (z1 - z2);
            grad_xyz1[((size_t)i * n + j) * 3 + 0] += gx;
            grad_xyz1[((size_t)i * n + j) * 3 + 1] += gy;
            grad_xyz1[((size_t)i * n + j) * 3 + 2] += gz;
            grad_xyz2[((size_t)i * m + j2) * 3 + 0] += -gx;
            grad_xyz2[((size_t)i * m + j2) * 3 + 1] += -gy;
            grad_xyz2[((size_t)i * m + j2) * 3 + 2] += -gz;
        }
    }
}

ORACLE_API int oracle_chamfer_backward(int b, int n, const float *xyz1, int m,
                                       const float *xyz2,
                                       const float *graddist1, const int *idx1,
                                       const float *graddist2, const int *idx2,
                                       float *gradxyz1, float *gradxyz2)
{
    nm_distance_grad(b, n, xyz1, m, xyz2, graddist1, idx1, gradxyz1, gradxyz2);
    nm_distance_grad(b, m, xyz2, n, xyz1, graddist2, idx2, gradxyz2, gradxyz1);
    return 1;
}

/* ------------------------------------------------------------------------
 * EMD forward (auction algorithm).
 * Follows loss_functions/emd/emd_cuda.cu:95-226 round by round; the host
 * sequence is emd_cuda.cu:256-269 and the input checks :236-249.  Caller
 * allocates and pre-initialises every buffer as emd_module.py:43-54 does
 * (assignment/assignment_inv = -1, everything else 0).
 *
 * Bid value (:142-146):  d = float( (3.0 - (double)sqrtf(s)) - (double)price )
 *   with s the fp32 squared distance (target minus query) in `fma_mode`.
 * Bid partition (:104-118,136-139,165-173): thread_per_unass threads split
 *   every 2048-tile between them and lane 0 of the group combines the partial
 *   (best, better, best_i) triples in thread order.  That only matters for WHICH
 *   of several exactly equal maxima is reported; it is restated literally so
 *   that index ties resolve as in the reference.
 * GetMax (:181-194) is racy on exact ties in the reference (last writer
 *   wins); here bidders are visited in ascending j, so the highest j inside
 *   the 1e-6 window wins.  Assign (:196-215) is visited in ascending j.
 * max_idx and bid persist across rounds exactly as in the reference.
 * The compaction kernels (:23-93) only build the list of unassigned points
 *   (in arbitrary order); unass_idx/unass_cnt/unass_cnt_sum/cnt_tmp are filled
 *   the way an in-order compaction would so that callers can inspect them.
 * ---------------------------------------------------------------------- */
static void emd_bid_one(int n, const float *p1, const float *xyz2,
                        const float *price, int thread_per_unass, float eps,
                        int fma_mode, int *bid_out, float *inc_out)
{
    const int batch = 2048;
    float x1 = p1[0], y1 = p1[1], z1 = p1[2];
    float best = -1e9f, better = -1e9f;
    int best_i = -1;
    for (int t = 0; t < thread_per_unass; t++) {
        float tb = -1e9f, tbb = -1e9f;
        int ti = -1;
        for (int k2 = 0; k2 < n; k2 += batch) {
            int end_k = (n < k2 + batch ? n : k2 + batch) - k2;
            int delta = (end_k + thread_per_unass - 1) / thread_per_unass;
            int l = t * delta;
            int r = (t + 1) * delta < end_k ? (t + 1) * delta : end_k;
            for (int k = l; k < r; k++) {
                const float *p2 = xyz2 + (size_t)(k + k2) * 3;
                float x2 = p2[0] - x1;
                float y2 = p2[1] - y1;
                float z2 = p2[2] - z1;
                float s = sqdist(x2, y2, z2, fma_mode);
                float d = (float)((3.0 - (double)sqrtf(s)) - (double)price[k + k2]);
                if (d > tb) {
                    tbb = tb;
                    tb = d;
                    ti = k + k2;
                } else if (d > tbb) {
                    tbb = d;
                }
            }
        }
        if (t == 0) {
            best = tb;
            better = tbb;
            best_i = ti;
        } else if (tb > best) {           /* :167-171 */
            better = best > tbb ? best : tbb;
            best = tb;
            best_i = ti;
        } else {                          /* :172 */
            better = better > tb ? better : tb;
        }
    }
    *bid_out = best_i;
    *inc_out = best - better + eps;
}

ORACLE_API int oracle_emd_forward(int b, int n, int m, const float *xyz1,
                                  const float *xyz2, float *dist,
                                  int *assignment, float *price,
                                  int *assignment_inv, int *bid,
                                  float *bid_increments, float *max_increments,
                                  int *unass_idx, int *unass_cnt,
                                  int *unass_cnt_sum, int *cnt_tmp,
                                  int *max_idx, float eps, int iters,
                                  int fma_mode)
{
    if (n != m) return -1;          /* emd_cuda.cu:236-239 */
    if (b > 512) return -1;         /* :241-244 */
    if (n % 256 != 0) return -1;    /* :246-249 */
    const int block_cnt = n / 256;

    for (int it = 0; it < iters; it++) {
        const int last = (it == iters - 1);
        /* clear / calc_unass_cnt / calc_unass_cnt_sum / calc_unass_idx, :23-93 */
        int run = 0;
        for (int i = 0; i < b; i++) {
            int c = 0;
            for (int j = 0; j < n; j++)
                if (assignment[(size_t)i * n + j] == -1)
                    unass_idx[run + c++] = j;
            unass_cnt[i] = c;
            cnt_tmp[i] = c;
            run += c;
            unass_cnt_sum[i] = run;
        }
        for (int i = 0; i < b; i++) {
            int U = unass_cnt[i];
            if (U == 0) continue;    /* :105-106 */
            const int *ulist = unass_idx + (unass_cnt_sum[i] - U);
            const float *X1 = xyz1 + (size_t)i * n * 3;
            const float *X2 = xyz2 + (size_t)i * n * 3;
            float *P = price + (size_t)i * n;
            int *A = assignment + (size_t)i * n;
            int *AI = assignment_inv + (size_t)i * n;
            int *BID = bid + (size_t)i * n;
            float *INC = bid_increments + (size_t)i * n;
            float *MAXI = max_increments + (size_t)i * n;
            int *MIDX = max_idx + (size_t)i * n;
            int unass_per_block = (U + block_cnt - 1) / block_cnt;   /* :108 */
            int thread_per_unass = 256 / unass_per_block;            /* :109 */
            /* Bid, :95-179 (bidders are independent within a round) */
#pragma omp parallel for schedule(static)
            for (int u = 0; u < U; u++) {
                int j = ulist[u];
                emd_bid_one(n, X1 + (size_t)j * 3, X2, P, thread_per_unass,
                            eps, fma_mode, &BID[j], &INC[j]);
            }
            for (int u = 0; u < U; u++) {       /* atomicMax, :176 */
                int j = ulist[u];
                if (INC[j] > MAXI[BID[j]]) MAXI[BID[j]] = INC[j];
            }
            /* GetMax, :181-194 (ascending j == ulist order) */
            for (int u = 0; u < U; u++) {
                int j = ulist[u];
                int bid_id = BID[j];
                float bid_inc = INC[j];
                float max_inc = MAXI[bid_id];
                if (bid_inc - 1e-6 <= max_inc && max_inc <= bid_inc + 1e-6)
                    MIDX[bid_id] = j;
            }
            /* Assign, :196-215 */
            for (int u = 0; u < U; u++) {
                int j = ulist[u];
                int bid_id = BID[j];
                if (last || MIDX[bid_id] == j) {
                    float bid_inc = INC[j];
                    int ass_inv = AI[bid_id];
                    if (!last && ass_inv != -1) A[ass_inv] = -1;
                    AI[bid_id] = j;
                    A[j] = bid_id;
                    P[bid_id] += bid_inc;
                    MAXI[bid_id] = -1e9f;
                }
            }
        }
    }
    /* CalcDist, :217-226: delta = xyz1 - xyz2[assignment] */
    for (int i = 0; i < b; i++)
        for (int j = 0; j < n; j++) {
            int k = assignment[(size_t)i * n + j];
            const float *p1 = xyz1 + ((size_t)i * n + j) * 3;
            const float *p2 = xyz2 + ((size_t)i * n + k) * 3;
            dist[(size_t)i * n + j] =
                sqdist(p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2], fma_mode);
        }
    return 1;
}

/* EMD backward, emd_cuda.cu:284-316: gradient for xyz1 only, one writer per j. */
ORACLE_API int oracle_emd_backward(int b, int n, const float *xyz1,
                                   const float *xyz2, float *gradxyz,
                                   const float *graddist, const int *idx)
{
    for (int i = 0; i < b; i++)
        for (int j = 0; j < n; j++) {
            const float *p1 = xyz1 + ((size_t)i * n + j) * 3;
            int j2 = idx[(size_t)i * n + j];
            const float *p2 = xyz2 + ((size_t)i * n + j2) * 3;
            float g = graddist[(size_t)i * n + j] * 2;
            float *o = gradxyz + ((size_t)i * n + j) * 3;
            o[0] += g * (p1[0] - p2[0]);
            o[1] += g * (p1[1] - p2[1]);
            o[2] += g * (p1[2] - p2[2]);
        }
    return 1;
}

/* ------------------------------------------------------------------------
 * Deterministic farthest-point sampling used to build fixtures
 * (SURVEY.md appendix B): fp32 squared distances in mode 0, start index 0,
 * first arg-max.  The reference calls fpsample.fps_sampling (main.py:21-22),
 * a third-party Rust extension with a RANDOM start index, so its subsample is
 * not reproducible; this is the build's deterministic counterpart.
 * ---------------------------------------------------------------------- */
ORACLE_API void oracle_fps_mode(int n, const float *xyz, int k, int fma_mode, int *out_idx);
ORACLE_API void oracle_fps(int n, const float *xyz, int k, int *out_idx)
{
    oracle_fps_mode(n, xyz, k, 0, out_idx);
}

ORACLE_API void oracle_fps_mode(int n, const float *xyz, int k, int fma_mode, int *out_idx)
{
    float *d = (float *)malloc(sizeof(float) * (size_t)n);
    for (int i = 0; i < n; i++) d[i] = INFINITY;
    int cur = 0;
    for (int s = 0; s < k; s++) {
        out_idx[s] = cur;
        float cx = xyz[cur * 3 + 0], cy = xyz[cur * 3 + 1], cz = xyz[cur * 3 + 2];
        float bestv = -1.0f;
        int besti = 0;
        for (int i = 0; i < n; i++) {
            float dd = sqdist(xyz[i * 3 + 0] - cx, xyz[i * 3 + 1] - cy,
                              xyz[i * 3 + 2] - cz, fma_mode);
            float v = d[i] < dd ? d[i] : dd;
            d[i] = v;
            if (v > bestv) {
                bestv = v;
                besti = i;
            }
        }
        cur = besti;
    }
    free(d);
}

/* oracle_fps_mode that also returns, per sample, the running minimum it had when it
 * was drawn (minima[0] = +inf: the start point is not drawn from anything).  This is
 * what the samplers record for the device-side check (csrc/fps_verify.hip). */
ORACLE_API void oracle_fps_minima(int n, const float *xyz, int k, int fma_mode, int *out_idx, float *minima)
{
    float *d = (float *)malloc(sizeof(float) * (size_t)n);
    for (int i = 0; i < n; i++) d[i] = INFINITY;
    int cur = 0;
    float curv = INFINITY;
    for (int s = 0; s < k; s++) {
        out_idx[s] = cur;
        minima[s] = curv;
        float cx = xyz[cur * 3 + 0], cy = xyz[cur * 3 + 1], cz = xyz[cur * 3 + 2];
        float bestv = -1.0f;
        int besti = 0;
        for (int i = 0; i < n; i++) {
            float dd = sqdist(xyz[i * 3 + 0] - cx, xyz[i * 3 + 1] - cy,
                              xyz[i * 3 + 2] - cz, fma_mode);
            float v = d[i] < dd ? d[i] : dd;
            d[i] = v;
            if (v > bestv) {
                bestv = v;
                besti = i;
            }
        }
        cur = besti;
        curv = bestv;
    }
    free(d);
}

/* The DEFINITION of a right sampling, checked step by step with no shortcuts
 * (n k distance evaluations): the first wrong step of (idx, minima), or -1.
 * Step 0: idx[0] is the start point 0.  Step j >= 1: idx[j] is a point of the
 * cloud, and after samples idx[0 .. j-1] have been applied to the running minima D
 * every point i has D_i < M_j, or D_i == M_j and i >= idx[j] (the FIRST arg-max),
 * and the sample itself has D == M_j exactly.  minima[0] is not read. */
ORACLE_API int oracle_fps_check(int n, const float *xyz, int k, int fma_mode, const int *idx, const float *minima)
{
    if (idx[0] != 0) return 0;
    float *d = (float *)malloc(sizeof(float) * (size_t)n);
    for (int i = 0; i < n; i++) d[i] = INFINITY;
    int wrong = -1;
    for (int j = 1; j < k && wrong < 0; j++) {
        const int prev = idx[j - 1];          /* (in the cloud: step j - 1 passed) */
        const float cx = xyz[prev * 3 + 0], cy = xyz[prev * 3 + 1], cz = xyz[prev * 3 + 2];
        for (int i = 0; i < n; i++) {
            float dd = sqdist(xyz[i * 3 + 0] - cx, xyz[i * 3 + 1] - cy,
                              xyz[i * 3 + 2] - cz, fma_mode);
            d[i] = d[i] < dd ? d[i] : dd;
        }
        const int s = idx[j];
        const float m = minima[j];
        if (s < 0 || s >= n) {
            wrong = j;
            break;
        }
        for (int i = 0; i < n; i++)
            if (!(d[i] < m || (d[i] == m && i >= s))) wrong = j;
        if (d[s] != m) wrong = j;
    }
    free(d);
    return wrong;
}
