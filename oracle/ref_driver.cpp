/*
 * ref_driver.cpp -- host side of the reference-kernel binaries (oracle/_ref/libgenpc_ref_m*.so).
 *
 * TEST INFRASTRUCTURE ONLY.  Own code.  The kernels themselves are NOT here: oracle/ref_build.py
 * cuts every __global__ / __device__ function out of the reference checkout's chamfer3D.cu and
 * emd_cuda.cu into .inc files under oracle/_ref/ at build time, and this file includes them under the CPU
 * stand-in of oracle/ref_simt.h.  What this file restates is the reference's HOST code:
 *   - the launch sequences (chamfer3D.cu:142-143, 184-185; emd_cuda.cu:256-269, 307).  Every
 *     REF_LAUNCH line below is compared with the `kernel<<<grid, block>>>` text of the reference
 *     by ref_build.py, in order, and the build fails when they differ;
 *   - the input checks of emd_cuda_forward (emd_cuda.cu:236-249);
 *   - the initial state emd_module.py:43-54 gives the auction's buffers.
 * `order` selects the schedule (0 ascending, 1 descending; ref_simt.h).
 */
#include "ref_simt.h"

namespace ref_chamfer {
#include "_ref/chamfer_kernels.inc"
}
namespace ref_emd {
#include "_ref/emd_kernels.inc"
}

#define REF_API extern "C" __attribute__((visibility("default")))
#define REF_LAUNCH(kernel, grid, block, ...) \
    ok &= ref_simt::launch(grid, block, (ref_simt::Order)order, [&] { kernel(__VA_ARGS__); })

REF_API int ref_arith_mode(void) { return GENPC_REF_MODE; }

/* chamfer_cuda_forward: results are allocated as zeros by the caller (dist_chamfer_3D.py:33-37) */
REF_API int ref_chamfer_forward(int batch_size, int n, const float *xyz1, int m, const float *xyz2,
                                float *dist1, int *idx1, float *dist2, int *idx2, int order)
{
    int ok = 1;
    REF_LAUNCH(ref_chamfer::NmDistanceKernel, dim3(32,16,1), 512, batch_size, n, xyz1, m, xyz2, dist1, idx1);
    REF_LAUNCH(ref_chamfer::NmDistanceKernel, dim3(32,16,1), 512, batch_size, m, xyz2, n, xyz1, dist2, idx2);
    return ok;
}

/* chamfer_cuda_backward; gradxyz* are zeroed by the caller (dist_chamfer_3D.py:56-57).  wide1/wide2
 * (may be null) receive the float64 sums of the kernels' fp32 terms. */
REF_API int ref_chamfer_backward(int batch_size, int n, const float *xyz1, int m, const float *xyz2,
                                 const float *graddist1, const int *idx1, const float *graddist2,
                                 const int *idx2, float *gradxyz1, float *gradxyz2, double *wide1,
                                 double *wide2, int order)
{
    int ok = 1;
    if (wide1) ref_simt::wide_begin(gradxyz1, (size_t)batch_size * n * 3, wide1);
    if (wide2) ref_simt::wide_begin(gradxyz2, (size_t)batch_size * m * 3, wide2);
    REF_LAUNCH(ref_chamfer::NmDistanceGradKernel, dim3(1,16,1), 256, batch_size, n, xyz1, m, xyz2, graddist1, idx1, gradxyz1, gradxyz2);
    REF_LAUNCH(ref_chamfer::NmDistanceGradKernel, dim3(1,16,1), 256, batch_size, m, xyz2, n, xyz1, graddist2, idx2, gradxyz2, gradxyz1);
    ref_simt::wide_end();
    return ok;
}

/* emd_cuda_forward.  Every buffer is the caller's; this function gives them the initial state of
 * emd_module.py:43-54 first.  unass_cnt / unass_cnt_sum / cnt_tmp hold 512 ints (:52-54). */
REF_API int ref_emd_forward(int batch_size, int n, int m, float *xyz1, float *xyz2, float *dist,
                            int *assignment, float *price, int *assignment_inv, int *bid,
                            float *bid_increments, float *max_increments, int *unass_idx,
                            int *unass_cnt, int *unass_cnt_sum, int *cnt_tmp, int *max_idx,
                            float eps, int iters, int order)
{
    if (n != m) return -1;
    if (batch_size > 512) return -1;
    if (n % 256 != 0) return -1;
    if (batch_size < 1 || n < 256) return 0;        /* an empty grid is a launch error on the GPU */

    for (size_t k = 0; k < (size_t)batch_size * n; k++) {
        dist[k] = 0;
        assignment[k] = -1;
        assignment_inv[k] = -1;
        price[k] = 0;
        bid[k] = 0;
        bid_increments[k] = 0;
        max_increments[k] = 0;
        unass_idx[k] = 0;
        max_idx[k] = 0;
    }
    for (int k = 0; k < 512; k++) unass_cnt[k] = unass_cnt_sum[k] = cnt_tmp[k] = 0;

    int ok = 1;
    for (int i = 0; i < iters; i++) {
        REF_LAUNCH(ref_emd::clear, 1, batch_size, batch_size, cnt_tmp, unass_cnt);
        REF_LAUNCH(ref_emd::calc_unass_cnt, dim3(batch_size, n / 256, 1), 256, batch_size, n, assignment, unass_cnt);
        REF_LAUNCH(ref_emd::calc_unass_cnt_sum, 1, batch_size, batch_size, unass_cnt, unass_cnt_sum);
        REF_LAUNCH(ref_emd::calc_unass_idx, dim3(batch_size, n / 256, 1), 256, batch_size, n, assignment, unass_idx, unass_cnt, unass_cnt_sum, cnt_tmp);
        REF_LAUNCH(ref_emd::Bid, dim3(batch_size, n / 256, 1), 256, batch_size, n, xyz1, xyz2, eps, assignment, assignment_inv, price, bid, bid_increments, max_increments, unass_cnt, unass_cnt_sum, unass_idx);
        REF_LAUNCH(ref_emd::GetMax, dim3(batch_size, n / 256, 1), 256, batch_size, n, assignment, bid, bid_increments, max_increments, max_idx);
        REF_LAUNCH(ref_emd::Assign, dim3(batch_size, n / 256, 1), 256, batch_size, n, assignment, assignment_inv, price, bid, bid_increments, max_increments, max_idx, i == iters - 1);
    }
    REF_LAUNCH(ref_emd::CalcDist, dim3(batch_size, n / 256, 1), 256, batch_size, n, xyz1, xyz2, dist, assignment);
    return ok;
}

/* emd_cuda_backward; gradxyz is zeroed by the caller (emd_module.py:83). */
REF_API int ref_emd_backward(int batch_size, int n, const float *xyz1, const float *xyz2,
                             float *gradxyz, const float *graddist, const int *idx, double *wide,
                             int order)
{
    if (batch_size < 1 || n < 256 || n % 256 != 0) return 0;
    int ok = 1;
    if (wide) ref_simt::wide_begin(gradxyz, (size_t)batch_size * n * 3, wide);
    REF_LAUNCH(ref_emd::NmDistanceGradKernel, dim3(batch_size, n / 256, 1), 256, batch_size, n, xyz1, xyz2, graddist, idx, gradxyz);
    ref_simt::wide_end();
    return ok;
}
