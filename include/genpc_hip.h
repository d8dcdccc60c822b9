/*
 * genpc_hip.h -- C ABI of libgenpc_hip.so, the MI355X (gfx950) implementation of
 * GenPC's geometric hot path.
 *
 * Every entry point takes raw DEVICE pointers, plain sizes and a HIP stream
 * (hipStream_t passed as void*; NULL = the legacy default stream, which is what
 * the reference launches on).  No torch / ATen types cross this boundary.
 *
 * Contract (same as the reference's pybind modules):
 *   - the CALLER allocates every buffer, outputs and scratch included;
 *   - fp32 clouds are row-major contiguous [B,N,3]; indices are int32;
 *   - launches are asynchronous on `stream`; nothing is retained after return;
 *   - return 1 = ok, 0 = HIP error (message on stderr, genpc_last_error()),
 *     -1 = invalid shape (EMD: n != m, B > 512, n % 256 != 0).
 *
 * Arithmetic mode: genpc_set_arith sets the process-wide default, genpc_set_arith_thread
 * an override for the calling host thread (< 0 removes it); genpc_get_arith returns what a
 * call made by this thread would use.  An entry point reads the mode once, at entry.
 *   GENPC_ARITH_FMA (default)  d = fma(dz,dz, fma(dx,dx, dy*dy))  -- the
 *       contraction nvcc's default -fmad=true applies to the reference's
 *       `x2*x2+y2*y2+z2*z2`;
 *   GENPC_ARITH_STRICT         d = (dx*dx + dy*dy) + dz*dz, no contraction.
 *   Both are bit-reproduced by oracle/genpc_oracle.c (fma_mode 1 / 0).
 */
#ifndef GENPC_HIP_H
#define GENPC_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define GENPC_ARITH_STRICT 0
#define GENPC_ARITH_FMA 1

/* Library / device ------------------------------------------------------- */
int genpc_abi_version(void);              /* bumps when a signature or a documented behaviour changes (28: genpc_hpr_plan added, GENPC_HPR_NOCULL keeps bits 128 and 512 only; 27: genpc_grid_*_probe added; 26: genpc_nn_plan added; 25: genpc_nn_seeded_step added; 24: genpc_icp_plan added; 23: genpc_pose_loss_grad_batch added; 22: genpc_chamfer_backward_ragged added; 21: genpc_nm_distance_ragged added; 20: genpc_mesh_sample added; 19: genpc_uhd added; 18: genpc_knn_query added;
                                           * 17: genpc_fps_tune takes 0 or 256 only; 16: genpc_hpr_* asynchronous, counts -1 on an internal error;
                                           * genpc_fps*: out_idx[0] -2 = failed the check).
                                           * genpc_uhd_ragged came without a bump.  From 27 on an addition that changes no existing signature and no
                                           * documented behaviour no longer bumps the number: genpc_knn_mean_distance_ragged and
                                           * genpc_outlier_filter_ragged came that way, and so did genpc_knn_query_ragged (additive: the number
                                           * stays 27) and genpc_emd_forward_ragged / genpc_emd_backward_ragged (additive as well: still 27);
                                           * genpc_voxel_down_sample_ragged, genpc_icp_batch_ragged and genpc_icp_ragged_plan likewise: still 28;
                                           * genpc_scale_search_scores_ragged and genpc_scale_search_ragged_plan too: still 28;
                                           * genpc_pose_optimize_ragged, genpc_pose_loss_grad_ragged and genpc_pose_ragged_plan as well: still 28;
                                           * genpc_nn_ragged_tune and genpc_nn_ragged_dense_plan (the default search is unchanged): still 28;
                                           * genpc_render_points_ragged, genpc_render_points_ragged_backward and genpc_render_ragged_plan: still 28;
                                           * a missing symbol is found when the binding loads. */
const char *genpc_last_error(void);       /* last HIP error string, "" if none */
int genpc_set_arith(int mode);            /* process default; returns the previous one */
int genpc_set_arith_thread(int mode);     /* calling thread only, < 0: follow the default; returns the previous override */
int genpc_get_arith(void);
/* The calling host thread's modes -- genpc_set_arith_thread, genpc_nn_tune, genpc_emd_tune, genpc_pose_tune, genpc_fps_tune --
 * as eight ints, and their restoration in another thread: a caller that hands work to threads of its own (the lanes of
 * genpc_amd/pipeline.py) exports before it starts them and imports at the top of each.  Return the number of ints used. */
int genpc_thread_state_export(int out[8]);
int genpc_thread_state_import(const int in[8]);
/* The table of tuning / A-B switches: every switch is an environment variable GENPC_<NAME>, read once per process
 * through one function (csrc/common.hip: tune_env) that records it with its default and a line of documentation; none
 * changes a result.  Writes "NAME=value (default d) -- what" lines for the switches consulted so far into buf (at most
 * len bytes, NUL-terminated); returns the size the whole table needs (call with len 0 to size the buffer). */
int genpc_tune_table(char *buf, int len);
/* Frees the per-device scratch pool (split-target partials, EMD lists). */
int genpc_release_workspace(void);
/* Nearest-neighbour kernel selection, for tests and experiments: every path returns
 * the same bits.  path: 4 cell-sorted pruned exact search (two launches, O(N + M) work when most
 * queries have a target nearby; slower than the filters when many do not -- opt-in), 3 one-f16-MFMA
 * filter (default), 1 fp32-MFMA filter (default below ~6 M pairs), 0 VALU brute force, < 0 keep
 * (2 was the split-bf16 filter, removed in round 3: rejected).  hooks: bit mask of test hooks
 * (8: every query takes the exhaustive pass, 16: every listed tile is evaluated
 * exactly, 512: count what the filtered paths do, see genpc_nn_stats, 2048 / 4096: duplicate pre-pass of the f16
 * filter off / on whatever the policy says), < 0 keep.  Applies to calls made by the CALLING
 * host thread only (thread-local; other threads keep the defaults).  Returns the previous
 * path.  Environment (read once, at first use): GENPC_NN_PATH (valu | mfma32 | f16 |
 * grid), GENPC_NN_DEBUG.                                                         */
int genpc_nn_tune(int path, int hooks);
/* Counters of the filtered nearest-neighbour paths, accumulated on the current device
 * while hook 512 is set: out[0] queries answered, out[1] queries re-done by the exhaustive
 * pass (filter proof failed: exact ties, non-finite input), out[2] exact re-evaluations of
 * 16-/32-target pieces.  Synchronises `stream`; reset != 0 zeroes them afterwards.      */
int genpc_nn_stats(unsigned long long out[3], int reset, void *stream);
/* The plan (csrc/nn_plan.h) that genpc_chamfer_forward (ndir 2) or genpc_nm_distance (ndir 1) of [b, n, 3] against [b, m, 3]
 * would get on the calling thread, its genpc_nn_tune family and the process's GENPC_NN_* switches in force, on a device of
 * `cus` compute units; cus <= 0: the current device's, cus > 0: no GPU is touched.  Which kernel form a shape reaches depends
 * on the device: tests ask here instead of assuming.
 *   out[0] family (genpc_nn_tune's numbers)     out[1] form of the f16 filter's blocks: 0 four waves, 1 four waves at three
 *   blocks per CU, 2 four waves with the 2048-target LDS tile, 3 eight waves ("wide")
 *   out[2] 32-query tiles per wave Q (VALU family: queries per lane R)     out[3] target tiles per bookkeeping unit
 *   out[4] lists per lane     out[5] targets per slice     out[6], out[7] slices of direction 0, 1
 *   out[8] blocks of the first launch     out[9] blocks of the finish launch     out[10] 1: the finish kernel's EARLY form
 *   out[11] 1: too large for one launch (the call would fail)     out[12], out[13] query blocks per slice of direction 0, 1
 *   out[14] finish blocks per re-do report     out[15] the compute units planned for
 * Fields that a family does not have are 0; the cell search (family 4) has none.  Returns 1, -1 for a bad argument.     */
int genpc_nn_plan(int b, int n, int m, int ndir, int cus, int out[16]);
/* Exact-duplicate pre-pass of the filtered nearest-neighbour path (csrc/nn_dedupe.hip): mask[e][k / 32] bit k % 32 is set
 * iff point k of cloud e has bit-identical coordinates to a point of lower index in the same cloud -- such a target can
 * never be reported by the reference's first-index-wins scan (chamfer3D.cu:30-71).  xyz [b, n, 3] float, mask
 * [b, ceil(n / 32)] uint32 (device, every word written).  The nearest-neighbour entry points run it by themselves where
 * it pays (hooks 2048 / 4096 of genpc_nn_tune force it off / on); exposed for tests.  Returns 1 / 0 / -1.            */
int genpc_nn_duplicate_mask(int b, int n, const float *xyz, unsigned *mask, void *stream);
/* Kernel-level timing for bench.py: while enabled, HIP events bracket the filter kernel
 * (nn_f16_kernel) of every nearest-neighbour call THE CALLING HOST THREAD makes, on the call's stream
 * (the switch and the events are per thread: other threads' launches are untouched).  Returns the
 * duration in ms of the last bracketed launch (-1 if none), then sets the switch to `enable`. */
float genpc_nn_profile(int enable);

/* Chamfer3D -------------------------------------------------------------- *
 * Replaces chamfer_cuda_forward (loss_functions/Chamfer3D/chamfer3D.cu:136-154,
 * bound as chamfer_3D.forward in chamfer_cuda.cpp:17-19,31): for every point
 * of xyz1[B,N,3] the squared distance to, and index of, its nearest point in
 * xyz2[B,M,3] (dist1/idx1), and the converse (dist2/idx2).  Lowest index wins
 * ties.  The argument order is the one the reference keeps in its commented-out
 * raw-pointer prototype (chamfer3D.cu:135).                                  */
int genpc_chamfer_forward(int b, int n, const float *xyz1, int m,
                          const float *xyz2, float *dist1, int *idx1,
                          float *dist2, int *idx2, void *stream);

/* One direction only: result[B,N], result_i[B,N] for queries xyz[B,N,3] against
 * targets xyz2[B,M,3].  This is NmDistanceKernel itself (chamfer3D.cu:12-134);
 * the partial-matching losses (utils/loss_util.py:35-43) only consume this half. */
int genpc_nm_distance(int b, int n, const float *xyz, int m, const float *xyz2,
                      float *result, int *result_i, void *stream);

/* Nearest neighbour with a search limit -- what the reference asks of open3d's KD-tree in
 * remove_close_points (reg_xyz.py:41-52: search_knn_vector_3d(point, 1), keep the point unless the
 * returned SQUARED distance is below the threshold): queries whose nearest target lies within
 * radius2 (squared distance, <=) get exactly what genpc_nm_distance returns; the others get
 * result = +inf, result_i = -1.  Runs on the cell-sorted search, which then never looks farther
 * than the limit: O(N + M) whatever the overlap of the two clouds.  Returns -1 for radius2 < 0. */
int genpc_nm_distance_within(int b, int n, const float *xyz, int m, const float *xyz2,
                             float radius2, float *result, int *result_i, void *stream);

/* Ragged NmDistance: c independent pairs of any sizes in one call.  Pair j has queries xyz[noff[j] .. noff[j+1]) and targets
 * xyz2[moff[j] .. moff[j+1]).  noff, moff: HOST arrays of c + 1 ascending ints, noff[0] = moff[0] = 0; they are copied before
 * the call returns and may be reused at once.  xyz [noff[c],3], xyz2 [moff[c],3], result [noff[c]] float, result_i [noff[c]] int:
 * device, packed in pair order.  result_i is the index INSIDE the pair's own target cloud.
 * Finite clouds: pair j's results are bit for bit what genpc_nm_distance(1, N_j, .., M_j, ..) returns for that pair alone
 * (the call's arithmetic mode, lowest index among targets at bit-equal distance).
 * Non-finite coordinates -- a deliberate departure from genpc_nm_distance, whose 512-target tile rule means nothing to a
 * search that does not tile that way: a query with a non-finite coordinate gets (NaN, -1); every query of a pair whose
 * TARGET cloud holds a non-finite coordinate gets (NaN, -1); the other pairs of the call are unaffected.  Decided on the
 * device.
 * A pair with N_j == 0 is legal and writes nothing (its targets are not looked at).  Returns 1 at once for c == 0 or no
 * queries in total (after the offsets have been checked); -1 with genpc_last_error set and nothing enqueued for c < 0, null
 * noff / moff with c > 0, noff[0] != 0 or moff[0] != 0, descending offsets, a pair with queries and no targets, a null device
 * pointer with work to do, or beyond the limits: c <= 384 pairs per call (the pair table travels in the kernel arguments)
 * and noff[c], moff[c] <= 2^28 points.
 * Asynchronous on `stream`: two launches whatever c is, scratch from the library's workspace, no copy, no host read-back,
 * no synchronisation (csrc/nn_ragged.hip).                                                                              */
int genpc_nm_distance_ragged(int c, const int *noff, const float *xyz, const int *moff, const float *xyz2,
                             float *result, int *result_i, void *stream);

/* The calling host thread's choice for EVERY ragged nearest-neighbour search -- genpc_nm_distance_ragged and the two searches of
 * a step of genpc_pose_optimize_ragged / genpc_pose_loss_grad_ragged: 0 the grid search (the default), 1 the dense search
 * (csrc/nn_ragged_dense.hip): every query of a pair against every target of it, one launch on the targets as they are packed,
 * no grid and no workspace at all.  The same bits, non-finite contract included; what differs is the cost, n_j m_j wherever the
 * points lie, where the grid search's depends on how far a query is from its nearest target.  Returns the previous value; any
 * other value returns -1 with genpc_last_error set and leaves the choice as it was.  A per-thread mode like genpc_pose_tune, with
 * no environment variable.  It is NOT part of genpc_thread_state_export: the eight ints are taken, and the lanes of
 * genpc_amd/pipeline.py make no ragged call -- a thread that wants the dense search sets it itself.
 * In dense mode a call is refused (-1, genpc_last_error names the limit, nothing enqueued, no pointer looked at beyond the null
 * check) for more than 2^36 pair evaluations, sum of N_j M_j, in one call, and for a pair with queries and more than 2^20
 * targets: one workgroup walks all targets of its pair.                                                                       */
int genpc_nn_ragged_tune(int search);
/* The plan of a dense call with these HOST offset tables (csrc/nn_ragged_dense_plan.h; no GPU is touched): out[0] work items
 * (workgroups), [1] threads per workgroup, [2] queries per item, [3] targets per LDS tile, [4] targets per wave's share of a
 * tile, [5] LDS bytes per workgroup, [6] / [7] the low / high 32 bits of the 64-bit count of pair evaluations.  [1] .. [5] are
 * constants and are filled whatever the table is.  Returns 1; -1 with genpc_last_error set for out == NULL, for what
 * genpc_nm_distance_ragged refuses of a table, and -- out filled all the same -- for a call the dense search refuses.        */
int genpc_nn_ragged_dense_plan(int c, const int *noff, const int *moff, int out[8]);

/* Replaces chamfer_cuda_backward (chamfer3D.cu:176-195, chamfer_3D.backward in
 * chamfer_cuda.cpp:22-26,32).  gradxyz1[B,N,3] / gradxyz2[B,M,3] must be zeroed
 * by the caller (dist_chamfer_3D.py:56-57); the kernel accumulates into them. */
int genpc_chamfer_backward(int b, int n, const float *xyz1, int m,
                           const float *xyz2, const float *graddist1,
                           const int *idx1, const float *graddist2,
                           const int *idx2, float *gradxyz1, float *gradxyz2,
                           void *stream);

/* Ragged Chamfer backward: both directions for the c pairs of a ragged batch, every gradient row summed in a stated order --
 * no floating-point atomic, the same bytes on every run, on every stream and wherever a pair stands in the call.
 * Clouds and HOST offset tables are packed as for genpc_nm_distance_ragged (xyz1 [noff[c],3], xyz2 [moff[c],3]); graddist1,
 * idx1 [noff[c]] and graddist2, idx2 [moff[c]] are packed like their clouds, idx1 counted INSIDE the pair's own xyz2 slice and
 * idx2 inside its xyz1 slice, as the ragged forward returns them.  For pair j with slices A, B, g1, i1, g2, i2 of n and m rows,
 * per component in fp32, every product and sum rounded on its own (nothing is fused, whatever genpc_set_arith says):
 *     v(i) = (2 g1[i]) (A[i] - B[i1[i]])   present iff 0 <= i1[i] < m,        w(k) = (2 g2[k]) (B[k] - A[i2[k]])   present iff 0 <= i2[k] < n
 *     gradxyz1[i] = +0 + v(i), then + (-w(k)) for every k in ASCENDING order with i2[k] == i
 *     gradxyz2[t] = +0 + (-v(i)) for every i in ASCENDING order with i1[i] == t, then + w(t)
 * -- the order of the CPU oracle (direction 1 ascending, then direction 2 ascending), one of the schedules the rectangular
 * backward's atomics can produce.  An index outside its range (the forward's -1 for non-finite input) is skipped in both places
 * and never dereferenced; the other pairs of the call do not notice.
 * The call OVERWRITES every row of gradxyz1 [noff[c],3] and gradxyz2 [moff[c],3] (they need not be zeroed, unlike
 * genpc_chamfer_backward's); a row with no term is +0.0f.
 * Returns 1 at once for c == 0 or no rows at all (after the offsets have been checked); -1 with genpc_last_error set and nothing
 * enqueued for what genpc_nm_distance_ragged refuses, the offsets being checked in both roles: c < 0, c > 384, null or descending
 * offsets, noff[0] != 0 or moff[0] != 0, more than 2^28 points on a side, a pair that is empty on ONE side only (empty on both is
 * fine), a null device pointer with work to do.
 * Asynchronous on `stream`: a key kernel, one radix sort of the noff[c] + moff[c] (row, owner) pairs and a gradient kernel --
 * the number of launches does not depend on c; scratch from the library's workspace, the offsets travel in the kernel arguments,
 * no copy, no host read-back, no synchronisation (csrc/chamfer_grad_ragged.hip).                                              */
int genpc_chamfer_backward_ragged(int c, const int *noff, const float *xyz1, const int *moff, const float *xyz2,
                                  const float *graddist1, const int *idx1, const float *graddist2, const int *idx2,
                                  float *gradxyz1, float *gradxyz2, void *stream);

/* EMD (auction) ---------------------------------------------------------- *
 * Replaces emd_cuda_forward (loss_functions/emd/emd_cuda.cu:228-282, bound as
 * emd.forward in emd.cpp:12-17,27).  Same 14 caller-allocated buffers with the
 * same initial state as emd_module.py:43-54 (assignment/assignment_inv = -1,
 * the rest 0; unass_cnt/unass_cnt_sum/cnt_tmp are int32[512]).  On return:
 * dist[B,n] squared distance to the assigned point, assignment[B,n],
 * assignment_inv, price, bid, bid_increments, max_increments hold the
 * final auction state; max_idx is election scratch (the reference never resets it, emd_cuda.cu:181-194, and
 * no caller reads it: here every object that was bid for ends at -1); unass_idx/unass_cnt/unass_cnt_sum/cnt_tmp hold the
 * last round's compaction (order within unass_idx is unspecified, as in the
 * reference).                                                               */
int genpc_emd_forward(int b, int n, int m, const float *xyz1, const float *xyz2,
                      float *dist, int *assignment, float *price,
                      int *assignment_inv, int *bid, float *bid_increments,
                      float *max_increments, int *unass_idx, int *unass_cnt,
                      int *unass_cnt_sum, int *cnt_tmp, int *max_idx, float eps,
                      int iters, void *stream);

/* Implementation of genpc_emd_forward, for tests and A/B (applies to the calling host thread): 2 all rounds in ONE
 * launch whose threads own the points (csrc/emd_auction.hip; needs eps >= 0 and the whole launch resident: B n <= 3.5 x 256
 * x CUs, else the call falls back to 1), 1 a launch per round step with the cell-sorted culled bid (csrc/emd_grid.hip: a
 * bidder visits only the grid rows that can hold an object worth more than its current second-best), 0 the same with the
 * tiled bid over all objects, < 0 the default (2 when admitted; else 1 when eps >= 0 and n >= 4096 or B n >= 65536; else 0).
 * All give the same bits.  hooks (>= 0 to set; < 0 keep): 1 = count what the culled bid does (genpc_emd_stats; implies
 * the launch-per-round path).  Returns the previous setting. */
int genpc_emd_tune(int grid, int hooks);
/* Synchronises `stream` and returns 1 if a one-launch EMD call on it was abandoned since the last reset (its workgroups
 * did not all become resident within the spin bound; that call's dist is NaN), 0 if none, -1 on error. */
int genpc_emd_status(int reset, void *stream);
/* 1 = the calling host thread's last one-launch EMD call ran beside other streams' persistent launches -- the only situation in
 * which it can be abandoned (then genpc_emd_status() == 1 and dist is NaN); reading clears the flag; no device access.
 * genpc_amd/emd.py checks it behind every forward and repeats an abandoned call on the launch-per-round path. */
int genpc_emd_contended(void);
/* Counters of the culled bid, accumulated on the current device while hook 1 is set: out[0] bidder-rounds, out[1] rows
 * of their search boxes, out[2] rows kept by the bound, out[3] objects tested, out[4] exact (fp64) evaluations, out[5]
 * exact first-place ties (full re-scan), out[6] bidders without seeds (probe).  Synchronises `stream`; reset != 0 zeroes. */
int genpc_emd_stats(unsigned long long out[8], int reset, void *stream);

/* The CalcDist step alone (emd_cuda.cu:217-226): dist[B,n] = |xyz1[j] - xyz2[assignment[j]]|^2 (0 where assignment < 0). */
int genpc_emd_calc_dist(int b, int n, const float *xyz1, const float *xyz2, const int *assignment, float *dist, void *stream);

/* Replaces emd_cuda_backward (emd_cuda.cu:302-316, emd.backward in
 * emd.cpp:19-23,28): gradxyz[B,n,3] (caller-zeroed) += 2*graddist*(xyz1-xyz2[idx]). */
int genpc_emd_backward(int b, int n, const float *xyz1, const float *xyz2,
                       float *gradxyz, const float *graddist, const int *idx,
                       void *stream);

/* The auction over a RAGGED batch (csrc/emd_ragged.hip): c independent pairs, pair j of N_j points against N_j objects, in one
 * call.  off is a HOST array of c + 1 ints, ascending from 0, copied before return (it rides in the kernel arguments); one
 * table serves both clouds because the auction needs equal sizes inside a pair.  Every N_j is a multiple of 256, or 0.
 * Every device array is packed in pair order and off[c] long (x 3 for the points).  assignment and bid index inside the pair's
 * own objects, assignment_inv and max_idx inside its own points.  The outputs may arrive uninitialised: the call's first
 * launch writes every pair's initial state (emd_module.alloc_state's values) and the call's own scratch, so a second call on
 * the same buffers returns the same bits.
 * Contract: pair j's dist, assignment, assignment_inv, bid and bid_increments are bit for bit what
 * genpc_emd_forward(1, N_j, N_j, ...) returns on that pair alone from alloc_state's initial values, in the call's arithmetic
 * mode, for any eps (negative included) and any iters >= 0 (0: dist 0, assignment -1).  price is exact except after a forced
 * last round with several bidders on one object (the order of the additions there is a race in the reference too).  A point
 * whose own coordinates are not finite bids on object -1 in the reference and in genpc_emd_forward (an out-of-bounds write);
 * here it bids on object 0 of its pair.
 * Launches: at most 3 * iters + 2 whatever c is (as built: 2 * iters + 2 -- initial state, a bid and a resolve launch per
 * round, CalcDist); no host read-back, no synchronisation, no copy; no kernel waits for another workgroup.
 * Returns 1 when done or when there is nothing to do (c == 0, or no pair has points; a pair with N_j == 0 is legal and writes
 * nothing); 0 on a HIP error; -1 with genpc_last_error() set and nothing enqueued -- decided before the GPU is touched -- for
 * c < 0 or c > 384, a null off with c > 0, off[0] != 0 or descending offsets, an N_j that is not a multiple of 256,
 * off[c] > 2^28, iters < 0, or a null device pointer with work to do. */
int genpc_emd_forward_ragged(int c, const int *off, const float *xyz1, const float *xyz2,
                             float *dist, int *assignment, float *price, int *assignment_inv,
                             int *bid, float *bid_increments, float *max_increments, int *max_idx,
                             float eps, int iters, void *stream);
/* genpc_emd_backward per pair: gradxyz[off[c],3] (caller-zeroed) += 2 * graddist * (xyz1 - xyz2[idx]), idx inside the pair's
 * objects (an index outside them adds nothing).  The gradient goes to xyz1 only.  One launch; the same refusals. */
int genpc_emd_backward_ragged(int c, const int *off, const float *xyz1, const float *xyz2,
                              float *gradxyz, const float *graddist, const int *idx, void *stream);

/* Depth prompting: projection, splat, colour gather ------------------------ *
 * Replaces DepthPrompting.getUvs (DepthPrompting.py:239-271) for the cameras the
 * caller selects: view[C,12] are 3x4 row-major world->camera matrices (look-at,
 * camera looks down -Z: kaolin Camera.from_args, utils/camera_utils.py:143-147),
 * focal = 1/tan(fovy/2), near/far as kaolin's pinhole defaults (1e-2, 1e2).
 * Outputs uv[C,N,2], depth[C,N] (NDC z), optional transformed[C,N,3] (NULL to
 * skip) and optional bbox[C,4] = min_x, min_y, max_x, max_y of the NDC xy.
 * rescale != 0: uv = (xy - bbox centre) / max extent * padmul + 0.5 with
 * padmul = float(1 - 2*padding); else uv = (xy + 1) / 2.                       */
int genpc_get_uvs(int c, int n, const float *view, float focal, float znear,
                  float zfar, const float *xyz, float *transformed, float *uv,
                  float *depth, int rescale, float padmul, float *bbox,
                  void *stream);

/* (uv * res).long(), swapped to (row, col), clipped to [0, clip_max]
 * (DepthPrompting.py:179-184, ScaleAdapter.py:59-62).  pix[N,2] int32.          */
int genpc_uv_to_pixels(int n, const float *uv, float res, int clip_max, int *pix,
                       void *stream);

/* Replaces DepthPrompting.paintPixels (DepthPrompting.py:292-339): paints
 * colors[N,ch] into img[ch,res,res] IN PLACE with a (2*point_size-1)^2 square
 * stamp, no z-test; on collisions the highest point index wins (the reference's
 * CPU index_put order; undefined on its GPU path).  out[ch,res,res] receives the
 * vertically flipped image the reference returns.  owner[res*res] is int32
 * scratch.  Returns -1 on a non-positive res/ch/point_size.                     */
int genpc_paint_pixels(int res, int n, const int *pix, const float *colors, int ch,
                       int point_size, float *img, float *out, int *owner,
                       void *stream);

/* Replaces the Python loop of ScaleAdapter.colorPoint (ScaleAdapter.py:57-66):
 * out[N,ch] = img[:, h-1-row, col] (the image is read flipped top-bottom).      */
int genpc_gather_colors(int n, const int *pix, const float *img, int ch, int h,
                        int w, float *out, void *stream);

/* Everything of DepthPrompting.getDepth (DepthPrompting.py:100-237) after hidden-point removal, for c scans of different sizes
 * in one call (csrc/depth_prompt_ragged.hip).  off[c + 1]: HOST offsets, scan j owns the packed rows [off[j], off[j + 1]) of
 * xyz[T,3] and rgb[T,3] (device).  cams[c,2,12]: per scan the chosen view matrix and the opposite one.  vis: bytes, scan j's
 * block starts at 2 off[j] and is [2, n_j] -- what genpc_hpr_visibility writes for two eyes.  focal, znear, zfar, rescale and
 * padmul as genpc_get_uvs takes them; res the image side, point_size and mask_pixel_rate as getRawDepth takes them.
 * Per scan j: uv and depth through both cameras with the bits of genpc_get_uvs(2, n_j, ...) on that scan alone;
 * sums[j][r] (double) = the sum of (double) depth over the points visible in row r, in the order written down in
 * csrc/depth_prompt_ragged_plan.h, which depends on n_j alone (the same bits alone, anywhere in a batch, on every run; no
 * floating-point atomics); chosen[j] = sums[j][0] >= sums[j][1] ? 0 : 1; uv[T,2], depth[T], pix[T,2] (genpc_uv_to_pixels with
 * res and res - 1) and visible[T] (bytes) of the chosen row; images[c,4,3,res,res] = sparse_img, raw_depth, hole_mask1,
 * hole_mask2 of getRawDepth over the chosen row's visible points, in the vertically flipped form paintPixels returns (on a
 * pixel the highest point index wins; grey level 0.1 + 0.8 (1 - (d - dmin) / (dmax - dmin)) in float, every operation rounded
 * on its own, dmin / dmax the exact extremes of the visible depths; masks per channel).  status[j] = 1, or -1 for a scan
 * without points: nothing else of that scan is written and no other scan notices.  A scan that has points but none visible in a
 * row has that row's sum 0.0 exactly; with none visible in either row chosen[j] = 0 (by >=), status[j] = 1, uv, depth and pix of
 * row 0 are written as always, visible is all zero and the images are the paint of nothing: sparse_img = raw_depth =
 * hole_mask1 = 0 and hole_mask2 = 1 in every channel (this library's definition: the reference's getDepth raises there).
 * Asynchronous on `stream`: ONE memset and FOUR launches whatever c is, the table in the kernel arguments, scratch from the
 * library's workspace, integer atomics only, no copy, no read-back.  Returns 1 (c == 0 too); -1 with genpc_last_error set
 * ("genpc_depth_prompt_ragged: ...") and nothing enqueued for c < 0, c > GENPC_DEPTH_PROMPT_RAGGED_MAX_SCANS, res outside
 * [1, 4096], point_size or mask_pixel_rate < 1, point_size * mask_pixel_rate > 32, a null or ill-formed table, more than
 * 2^28 points, 2 c res^2 > 2^28, or a null required pointer.                                                             */
#define GENPC_DEPTH_PROMPT_RAGGED_MAX_SCANS 256
int genpc_depth_prompt_ragged(int c, const int *off, const float *xyz, const float *rgb, const float *cams,
                              const unsigned char *vis, float focal, float znear, float zfar, int rescale,
                              float padmul, int res, int point_size, int mask_pixel_rate, float *uv, float *depth,
                              int *pix, unsigned char *visible, int *chosen, double *sums, float *images,
                              int *status, void *stream);

/* What a genpc_depth_prompt_ragged call with this table and these settings does (csrc/depth_prompt_ragged_plan.h; no GPU is
 * touched): out[0] = workgroups of the per-point launches, out[1] = kernels, out[2] = memsets, out[3] = scans refused for
 * having no points, out[4] = the lowest of them (-1: none), out[5] = 32-bit words the memset fills, out[6] = scratch bytes.
 * Returns 1; -1 with genpc_last_error set for out == NULL or a call genpc_depth_prompt_ragged refuses.                    */
int genpc_depth_prompt_ragged_plan(int c, const int *off, int res, int point_size, int mask_pixel_rate,
                                   long long out[7]);

/* ScaleAdapter.colorPoint for c scans, each with its own image: imgs[c,ch,h,w]; uv[T,2] packed by the HOST table off[c + 1].
 * One launch: per scan, pix (optional, [T,2]) has the bits of genpc_uv_to_pixels(res, clip_max) and out[T,ch] those of
 * genpc_gather_colors on that scan and its image.  Returns 1; -1 with genpc_last_error set for c < 0, c > 256, a null or
 * ill-formed table, more than 2^28 points, clip_max outside [0, min(h, w)), or a null required pointer.                  */
int genpc_gather_colors_ragged(int c, const int *off, const float *uv, const float *imgs, int ch, int h, int w,
                               float res, int clip_max, int *pix, float *out, void *stream);

/* Replaces DepthPrompting.getVisiblePoints (DepthPrompting.py:273-290): open3d's
 * PointCloud.hidden_point_removal(camera, radius) for every viewpoint -- Katz' operator:
 * spherical flipping p' = v + 2 (radius - |v|) v / |v|, v = p - eye, then the vertices of
 * the convex hull of the flipped points and the origin.  Computed exactly, without a hull:
 * a flipped point is a vertex iff the polygon of normals (tilts of its own direction) that
 * keep every other flipped point below it is not empty (genpc_amd/csrc/hpr.hip; double
 * arithmetic; at most 4096 viewpoints and 2^31 - 1 (viewpoint, point) pairs per call).  points[N,3] float, eyes[C,3] DOUBLE (both
 * device), radius > 0; visible[C,N] bytes, counts[C].  second_pass_points (HOST int, may
 * be NULL): how many points the wave-per-point passes took over (lattice-like inputs: many).
 * Asynchronous: every pass reads its item count from device memory, nothing is fetched -- unless
 * second_pass_points is given, which costs the call's only stream synchronisation.  An internal error (none known)
 * cannot be returned without one either: it turns every count into -1.  Polygons of any size: up to 128 and
 * 1024 vertices in LDS, beyond that in global memory.  Differences from qhull: normals tilted more than atan(1e4) from
 * the point's direction are not considered; of exact duplicates (-0 == +0) only the copy with the
 * lowest index takes part -- qhull reports one copy of a coincident group too, so counts agree.     */
int genpc_hpr_visibility(int c, int n, const float *points, const double *eyes,
                         double radius, unsigned char *visible, int *counts,
                         int *second_pass_points, void *stream);

/* The same pass for a caller that only needs THE BEST view (DepthPrompting.viewpoint_select,
 * DepthPrompting.py:87-98: argmax over the viewpoints of the visible count): after the first polygon
 * kernel a view's count is a lower bound and the number of its still undecided points is known, so a
 * view whose upper bound stays below the best lower bound cannot win (nor tie) and its remaining
 * points are skipped.  counts[c]: exact for the views with exact[v] = 1 (exact may be NULL), a lower
 * bound below the maximum for the others -- argmax(counts) (first maximum) is the reference's choice.
 * visible[c,n] is complete only for the exact views.  Other arguments as genpc_hpr_visibility.       */
int genpc_hpr_best_view_counts(int c, int n, const float *points, const double *eyes, double radius,
                               unsigned char *visible, int *counts, unsigned char *exact,
                               int *second_pass_points, void *stream);

/* The plan of a hidden-point-removal call of c views x n points (csrc/hpr_plan.h; best_only: the call is
 * genpc_hpr_best_view_counts) on a device of `cus` compute units (<= 0: the current device's), with the process's
 * GENPC_HPR_* switches; no GPU work.  out[24]:
 *   out[0] 1: too large (the call would fail)     out[1] tiles per view     out[2] two-kernel form     out[3] views are pruned
 *   out[4] key bits of the view sort     out[5] clips before a polygon is handed over     out[6], out[7] home tiles, chunks
 *   out[8] candidates marked at a time     out[9], out[10] hand-over of a block's last points: from batch, at most lanes
 *   out[11] parked points the polygon store holds     out[12] 1: the first try has a kernel of its own
 *   out[13], out[14] 256-thread blocks over the points, capped     out[15] over the views
 *   out[16] .. out[19] one-wave blocks: first try, walk, large polygons, global polygons     out[20] vertices per global buffer
 *   out[21], out[22] MiB of the polygon store, of the global buffers (rounded down)     out[23] the compute units planned for
 * Returns 1, -1 for a bad argument.     */
int genpc_hpr_plan(int c, int n, int best_only, int cus, int out[24]);

/* A cheaper visibility for viewpoint ranking.  NOT the reference's operator (that is
 * genpc_hpr_visibility above): a z-buffer test -- a point is visible from camera c
 * when no point whose (2*point_size-1)^2 pixel stamp covers its pixel of a res x res
 * image is nearer by more than tol (NDC depth).  uv[C,N,2] / depth[C,N] as produced
 * by genpc_get_uvs; visible[C,N] bytes, counts[C] = visible points per camera.   */
int genpc_zbuffer_visibility(int c, int n, const float *uv, const float *depth,
                             int res, int point_size, float tol,
                             unsigned char *visible, int *counts, void *stream);

/* SE(3)+scale alignment ---------------------------------------------------- *
 * Pose model of ObjectPoseOptim.forward (optim_registration/diff_obj_pose.py:
 * 408-423): params[10] = rot_6d[6], trans[3], log_scale[1] (device memory),
 * pts = (R ((v - center) s)^T)^T + center + trans.                             */
int genpc_pose_transform(int n, const float *v, const float *center,
                         const float *params, float *pts, void *stream);

/* Chamfer half of compute_loss_function (diff_obj_pose.py:326-334) plus the
 * orthogonality term (:543-545) and its analytic gradient:
 *   loss = cd_weight * (mean sqrt(d1) + 0.5 mean sqrt(d2)) + reg_weight * |RR^T-I|_F
 * with d1/i1 = NN of the transformed complete cloud in `partial` and d2/i2 the
 * converse (one genpc_chamfer_forward call).  loss_out[3] = loss, cd, |RR^T-I|_F;
 * grad[10] in parameter order.  All pointers are device memory.                 */
int genpc_pose_cd_grad(int nc, const float *v, const float *center,
                       const float *params, int np, const float *partial,
                       const float *d1, const int *i1, const float *d2,
                       const int *i2, float cd_weight, float reg_weight,
                       float *loss_out, float *grad, void *stream);

/* The multi-start Adam loop of object_pose_optimization (diff_obj_pose.py:516-594)
 * with the Chamfer half of its loss: `starts` initial rotations R_y(90 deg * k),
 * iters+1 Adam steps each (lr, 0.2 lr, 0.1 lr for rot/trans/log-scale), best start
 * by lowest loss seen keeps its FINAL parameters.  Writes transform[16] =
 * [[sR, t],[0,1]] row-major, history[starts*(iters+1)] (optional) and
 * best_params[10] (optional); device memory, no host synchronisation.           */
int genpc_pose_optimize_cd(int nc, const float *complete, int np,
                           const float *partial, float lr, int iters, int starts,
                           float *transform, float *history, float *best_params,
                           void *stream);

/* The same loop for B scans in lock-step: complete[B,nc,3], partial[B,np,3],
 * transform[B,16], history[B,starts*(iters+1)] (optional), best_params[B,10]
 * (optional).  One batched NN launch per step serves all B scans.               */
int genpc_pose_optimize_cd_batch(int b, int nc, const float *complete, int np,
                                 const float *partial, float lr, int iters,
                                 int starts, float *transform, float *history,
                                 float *best_params, void *stream);

/* Silhouette ("mask") half of the pose loss -------------------------------------- *
 * The reference compares PulsarPointsRenderer images (pytorch3d, CUDA only -- absent here and
 * unpinned) of the partial cloud with its colours (diff_obj_pose.py:108-134; load_point_cloud
 * returns vert_col for every input the pipeline produces, :136-164) and of the posed complete cloud
 * with its colours (:426-433).  This library draws both with its OWN differentiable colour splat, same
 * camera (eye (0,0,3) looking at the origin, focal 4 NDC) and radii (world units):
 *   Zv = 3 - z;  u = S/2 (1 + 4 x / Zv);  v = S/2 (1 - 4 y / Zv);  rho = S/2 * 4 * radius / Zv
 *   a_i = min(0.999, max(0, 1 - |pixel centre - (u, v)|^2 / rho^2))
 *   O = 1 - prod_i (1 - a_i);  A_ch = sum_i a_i c_i,ch / sum_i a_i;  img_ch = O * A_ch
 * (coverage-weighted colour, order-independent; Pulsar's softmax in depth is NOT reproduced).
 * genpc_splat_image writes img[size, size, 3] (H, W, C like the reference's renders, row 0 at the
 * top) for pts[n,3] with colours col[n,3] in [0,1]; col == NULL draws white (what load_point_cloud
 * substitutes when a PLY has no colours, :157-158).                                              */
int genpc_splat_image(int n, const float *pts, const float *col, float radius, int size,
                      float *img, void *stream);

/* compute_loss_function's mask terms on given images (diff_obj_pose.py:286-311 with
 * normalize_images :204-217, compute_soft_mask :261-278, dice_loss :238-259): img, ref [size,size,3]
 * device float32 -> loss_out[1] = 30 MSE + BCE + 10 Dice of the luminance soft masks after the
 * per-channel statistical normalisation of img towards ref; grad (NULL to skip) [size,size,3] =
 * d loss / d img.  The same device code as the alignment loop's; pinned to the reference's own
 * Python through tests/golden/ref_py_mask_loss.npz.  Returns 1 / 0 / -1 (size < 2).               */
int genpc_mask_loss(int size, const float *img, const float *ref, float *loss_out, float *grad,
                    void *stream);

/* compute_loss_function as a whole (diff_obj_pose.py:286-336) + the orthogonality term, and its
 * analytic gradient:
 *   loss = mask_weight * mask_loss + cd_weight * cd + reg_weight * |RR^T - I|_F
 *   mask_loss = 30 MSE(m, m_ref) + BCE(m, m_ref) + 10 Dice(m, m_ref)  on the soft masks
 *   m = sigmoid((luminance of the normalised image - 0.1) / 0.05) of the posed cloud (colours
 *   vert_col[nc,3], splat radius 1.1 * radius, :385) and of `partial` (colours partial_col[np,3],
 *   radius, :118); per-channel statistical normalisation as at :204-217.  NULL colours = white.
 * d1/i1/d2/i2 as in genpc_pose_cd_grad.  mask_weight = 0 skips the mask term (render_size, radius
 * and the colours are then ignored).  loss_out[4] = loss, cd, |RR^T-I|_F, mask_loss; grad[10].   */
int genpc_pose_loss_grad(int nc, const float *v, const float *vert_col, const float *center,
                         const float *params, int np, const float *partial,
                         const float *partial_col, const float *d1, const int *i1,
                         const float *d2, const int *i2, float cd_weight, float reg_weight,
                         float mask_weight, float radius, int render_size, float *loss_out,
                         float *grad, void *stream);

/* The same loss and gradient for b elements in one call, each with its own clouds, centre and parameters, evaluated with
 * the launches ONE STEP of genpc_pose_optimize_batch makes at b elements on one stream (no Adam step is taken): the fused
 * transform + projection, the bidirectional nearest-neighbour search (so no d1 / i1 / d2 / i2 are passed; without the loop's
 * once-per-call duplicate masks -- the search makes its own where it wants them, the results are the same bits), the Chamfer
 * gradient as a launch of its own or inside the silhouette gradient's, the silhouette step, the per-element finish -- every
 * launch width from csrc/pose_plan.h (an ask of b scans, one start, no side stream, the GENPC_POSE_* switches at their
 * defaults).  What the plans select for wide calls -- one lane per point, whole images per XCD, at most 24 blocks per element
 * in the Chamfer gradient from 16 elements on, more than one block of per-element threads above 64 elements -- is thereby
 * comparable with an independent reference element by element.
 *   v [b,nc,3], vert_col [b,nc,3] or NULL, center [b,3], params [b,10], partial [b,np,3], partial_col [b,np,3] or NULL
 *   -> loss_out [b,4] = loss, cd, |RR^T-I|_F, mask_loss;  grad [b,10].
 * mask_weight = 0: the Chamfer-only objective (render_size, radius and the colours are ignored).
 * Returns 1 / 0 / -1 (b, nc or np <= 0; with a mask term: render_size <= 1 or radius not positive).  Asynchronous on `stream`;
 * scratch from a workspace slot of its own.  genpc_pose_loss_grad remains the single-element evaluation with the caller's
 * neighbours and the projection inside the splat's launch pair. */
int genpc_pose_loss_grad_batch(int b, int nc, const float *v, const float *vert_col, const float *center,
                               const float *params, int np, const float *partial,
                               const float *partial_col, float cd_weight, float reg_weight,
                               float mask_weight, float radius, int render_size, float *loss_out,
                               float *grad, void *stream);

/* The renderer of the mask term (genpc_splat_image, genpc_pose_loss_grad, genpc_pose_loss_grad_batch, genpc_pose_optimize_batch), per calling host thread:
 * 1 = Pulsar's published blending function (Lassner & Zollhoefer, CVPR 2021, eq. 1-2) with the reference's arguments
 *     (diff_obj_pose.py:126-131,428-433: gamma 1e-2, znear 1e-4, zfar 5, bg 0): over the discs covering a pixel
 *       I_ch = sum_i a_i e_i c_i,ch / (B + sum_i a_i e_i),  e_i = exp(z_i / gamma),  z_i = (zfar - Zv_i) / (zfar - znear),  B = exp(1e-10 / gamma)
 *     with the coverage a_i and the camera of the splat above -- a near surface hides a far one.  THE DEFAULT.  What of it is
 *     from memory (pytorch3d is absent and unpinned) is listed in oracle/genpc_oracle_geom.c;
 * 0 = the coverage splat described above (order-independent: front and back surfaces are averaged; rounds 2-4);
 * < 0 = back to the default.  Returns the previous setting (-1 = default). */
int genpc_render_tune(int blend);

/* The renderer as a differentiable operation of its own: b clouds of n points drawn in one call, and the backward of those images
 * for a caller's d L / d img, per point (csrc/render_grad.hip; genpc_amd.optim_registration.diff_obj_pose.render_points is the
 * torch.autograd.Function over the pair).  The camera is the one above; radius is used as given (a caller who draws the posed
 * cloud applies the reference's factor 1.1 itself, like genpc_splat_image's).
 *   pts [b,n,3], col [b,n,3] or NULL (white), img / grad_img [b,size,size,3], planes [b,5,size*size],
 *   grad_pts [b,n,3], grad_col [b,n,3] or NULL (not computed; it may be asked for with col == NULL).
 * blend (0 or 1) is an ARGUMENT, not the calling thread's genpc_render_tune mode: torch runs a backward on an autograd engine
 * thread, where a mode the forward's thread set is not visible.  (Inside, the thread's mode is saved, set and restored around the
 * launches; genpc_splat_image and every other call keep reading the thread's mode.)
 * genpc_render_points: element e of img is bit for bit genpc_splat_image of element e alone under that blend.  planes_out (NULL to
 *   skip) receives the five planes the images were made from -- blend 0: T, D, N_r, N_g, N_b; blend 1: m, D', N'_r, N'_g, N'_b
 *   (csrc/mask.h).  n == 0 draws the background.
 * genpc_render_points_backward: two launches, no atomics, no workgroup that waits for another; the same bits in every run, on every
 *   stream and in every batch.  Per pixel, with G = grad_img:
 *     blend 1:  W1 = m,  W4 = (G, G . I) / D';      blend 0:  W1 = T (G . A),  W4 = (O / D) (G, G . A),  1 / D := 0 where D = 0.
 *   Per point, over the pixel centres of its disc's box in a fixed order (eight lanes a point, rows interleaved, columns ascending,
 *   a fixed tree over the eight), gu, gv, grho, gz as the silhouette loss's own gather forms them, then
 *     grad_pts = (gu f4 / Zv, -gv f4 / Zv, -gZv),   f4 = 4 size / 2,
 *     grad_col[ch] = sum over the pixels with a > 0 of W4.ch min(a, 0.999) exp(ze - W1)  (blend 1),  W4.ch min(a, 0.999)  (blend 0).
 *   Pixels where the coverage is clamped (a >= 0.999) count for the colour and for the depth term gz, not for gu, gv, grho.
 *   A point the camera does not see, or one with a coordinate that is not finite, gets +0 rows.  n == 0: nothing is written.
 *   THE PLANES CONTRACT: `planes` must be what genpc_render_points returned in planes_out for the same pts, col, radius, size and
 *   blend.  Blend 1 evaluates exp(ze - m) with m the pixel's largest exponent; it is <= 1 only for the planes of these very points
 *   and overflows for others.  No gradient with respect to the radius or the camera; no double backward.
 * Both return 1, 0 (a runtime error, genpc_last_error) or -1 with genpc_last_error set and NOTHING enqueued: b <= 0, n < 0,
 * size <= 0 (or > 8192), a radius that is not positive, blend outside {0, 1}, b * n or b * size * size beyond 2^28, or a null pts, img,
 * planes, grad_img or grad_pts with work to do.
 * Asynchronous on `stream`; scratch from workspace slots of their own. */
int genpc_render_points(int b, int n, const float *pts, const float *col, float radius, int size, int blend,
                        float *img, float *planes_out, void *stream);
int genpc_render_points_backward(int b, int n, const float *pts, const float *col, float radius, int size, int blend,
                                 const float *planes, const float *grad_img,
                                 float *grad_pts, float *grad_col, void *stream);

/* The same pair for s clouds of DIFFERENT sizes, each drawn with a radius of its own, in one call (csrc/render_grad.hip, shape:
 * csrc/render_ragged_plan.h; genpc_amd.optim_registration.diff_obj_pose.render_points_ragged is the torch.autograd.Function over it,
 * and maps other pinhole cameras onto the library's one by an affine map of the points and a scaling of the radius).
 *   off: HOST, s + 1 ints from 0, ascending (element j owns points [off[j], off[j + 1]); an element may be empty);
 *   radius: HOST, s floats; pts [off[s],3], col [off[s],3] or NULL (white), img / grad_img [s,size,size,3], planes [s,5,size*size],
 *   grad_pts [off[s],3], grad_col [off[s],3] or NULL (not computed).
 * Element j of img, planes_out, grad_pts and grad_col is BIT FOR BIT what genpc_render_points / genpc_render_points_backward give for
 * b = 1 on element j alone with radius[j] -- the same bytes in every run, on every stream, wherever the element stands in the list and
 * whatever its neighbours are.  An empty element's image is the background (b = 1, n = 0) and it has no gradient rows.  The planes
 * contract above holds per element.  The backward uses no atomics and no workgroup waits for another.
 * Neither host table is read after the call returns: both travel by value in a kernel's arguments, which bounds a call at
 * GENPC_RENDER_RAGGED_MAX_ELEMENTS = 384 elements (a longer list goes in several calls).  Per-element limits are
 * genpc_render_points' own.
 * Both return 1, 0 (a runtime error) or -1 with genpc_last_error set, NOTHING enqueued and nothing written: s <= 0 or s > 384, a null
 * off or radius, size outside 1 .. 8192, blend outside {0, 1}, a table that does not start at 0 or descends, a radius that is not
 * positive (named by its element), off[s] or s * size * size beyond 2^28, or a null pts, img, planes, grad_img or grad_pts with work
 * to do.  A backward of a list without points returns 1 and writes nothing.
 * genpc_render_ragged_plan: the plan both read (no GPU is touched), out = { the bound on s, the element a refusal names or -1, s, the
 *   largest element, off[s], size * size, the projection's blocks per element, the per-pixel kernels' blocks per image, the gather's
 *   blocks per element, the gather's blocks, the per-element count that sizes the projected points' scratch, s * size * size };
 *   -1 with the refusal recorded as the forward would. */
#define GENPC_RENDER_RAGGED_MAX_ELEMENTS 384
int genpc_render_points_ragged(int s, const int *off, const float *pts, const float *col, const float *radius, int size, int blend,
                               float *img, float *planes_out, void *stream);
int genpc_render_points_ragged_backward(int s, const int *off, const float *pts, const float *col, const float *radius, int size,
                                        int blend, const float *planes, const float *grad_img,
                                        float *grad_pts, float *grad_col, void *stream);
int genpc_render_ragged_plan(int s, const int *off, const float *radius, int size, int blend, int out[12]);

/* Nearest-neighbour path of genpc_pose_optimize_batch, for tests and A/B (applies to the calling host thread): 1 the
 * seeded cell search from the second Adam step on (csrc/nn_seeded.hip: every query starts from last step's answer and
 * searches only the ball it leaves; grids built once per call, the moving cloud's in its rest frame), 0 the brute-force
 * filter at every step (on real shapes three of the four starts are misaligned, most of their queries have no near
 * target and the seeded search loses), 2 measure both during the call and take the faster one (the default: a few
 * hipEventSynchronize per call on the call's stream), < 0 the default / environment GENPC_POSE_SEEDED.  Same bits in
 * every mode for finite clouds (a NaN coordinate: see the head of csrc/nn_seeded.hip).  Returns the previous setting.
 * Where it is tested: the loop's fp32 loss histories are identical in modes 0, 1 and 2 (tests/test_gpu_determinism.py), and
 * the seeded search itself is held to the reference's (distance, first index) query by query, bit for bit, through
 * genpc_nn_seeded_step below (tests/test_gpu_nn_seeded.py; its inputs: tests/nn_seeded_cases.py). */
int genpc_pose_tune(int seeded);
/* ONE step of the seeded search on the caller's inputs, with the loop's own functions in the loop's order: both grids built
 * (the static clouds' in the world frame, the rest clouds' in the rest frame), posed = the transform of rest by (center, params)
 * at the loop's launch width, then one seeded launch with i1 / i2 as the seeds (any int: a value outside [0, count) is no
 * seed) -- in the calling thread's arithmetic mode.
 *   rest [b,nm,3], center [b,3], params [b,10], stat [b,ns,3]  ->  posed [b,nm,3];
 *   d1, i1 [b,nm]: every posed point's nearest static point;  d2, i2 [b,ns]: every static point's nearest posed point.
 * sample > 1: the loop's timing probe -- only every sample-th block of 64 queries runs (blocks numbered over direction 1's
 * b * ceil(nm / 64), then direction 2's b * ceil(ns / 64)); the other queries' outputs are left as they were.
 * Returns 1 / 0 / -1 (b, nm or ns <= 0, sample < 1: nothing is written).  Asynchronous on `stream`; scratch from a workspace
 * slot of its own. */
int genpc_nn_seeded_step(int b, int nm, const float *rest, const float *center, const float *params,
                         int ns, const float *stat, float *posed, float *d1, int *i1, float *d2,
                         int *i2, int sample, void *stream);
/* The calling host thread's alignment loops (full objective, small clouds): 1 = the Chamfer half of an Adam step -- nearest
 * neighbours + gradient -- on a side stream of the highest priority class beside the silhouette half, 0 = one stream,
 * < 0 = default (GENPC_POSE_DUAL, on).
 * Same results either way.  Returns the previous setting. */
int genpc_pose_dual(int on);

/* object_pose_optimization's loop with the FULL objective for B scans in lock-step: as
 * genpc_pose_optimize_cd_batch plus, per Adam step, the splat of the posed cloud, the mask loss
 * and its gradient (four more launches; the reference image of `partial` is drawn once).
 * complete_col[B,nc,3] / partial_col[B,np,3]: the clouds' colours in [0,1] (vert_col of
 * load_point_cloud, :136-164), NULL = white.  radius / render_size: diff_obj_pose.py:496;
 * mask_weight 1 is the reference's weight (:331).                                                 */
int genpc_pose_optimize_batch(int b, int nc, const float *complete, const float *complete_col,
                              int np, const float *partial, const float *partial_col, float lr,
                              int iters, int starts, float radius, int render_size,
                              float mask_weight, float *transform, float *history,
                              float *best_params, void *stream);

/* The alignment loop for c scans of DIFFERENT sizes in one call (the ragged form; csrc/pose_ragged_plan.h has its shape).
 * coff / poff [c + 1] are HOST offset tables into the packed device clouds complete[coff[c],3] and partial[poff[c],3] (colours
 * packed alike, NULL = white); they travel by value in kernel arguments, nothing of them is read after return.
 *   -> transform[c,16], history[c, starts*(iters+1)] or NULL (row = start, as genpc_pose_optimize_batch), best_params[c,10] or NULL.
 * Scan j's results are those of genpc_pose_optimize_batch(1, nc_j, ...) on scan j alone wherever it stands in the batch, within
 * the tolerances tests/test_gpu_pose_ragged_loop.py states: the same objective, renderer (genpc_render_tune), arithmetic mode,
 * start rotations, patience rule and pick-the-best-start rule -- the same device functions, given an element table.  What differs
 * is the simple shape of the loop: the starts side by side as batch elements (element = scan * starts + start), ONE stream,
 * the Adam update a launch of its own, nearest neighbours from genpc_nm_distance_ragged's grid search in both directions (the
 * bits of genpc_nm_distance per element; the partial clouds' grids are built once per call, the posed clouds' every step).
 * A call holds at most GENPC_POSE_RAGGED_MAX_ELEMENTS = 384 elements (96 scans at 4 starts) and 2^28 points per side, starts
 * included.  Returns 1 (also for c = 0: nothing written), 0 on a HIP error; -1 with genpc_last_error set
 * ("genpc_pose_optimize_ragged: ...") and nothing enqueued for c < 0, a null or ill-formed table, a scan with an EMPTY cloud on
 * either side (named by its number), more elements or points than a call holds ("more than 384 elements ..."), starts < 1,
 * iters < 0, a null pointer, or the full objective with render_size <= 1 or a radius that is not positive.  Asynchronous on
 * `stream`: no read-back, no synchronisation; scratch from workspace slots of its own. */
#define GENPC_POSE_RAGGED_MAX_ELEMENTS 384
int genpc_pose_optimize_ragged(int c, const int *coff, const int *poff, const float *complete,
                               const float *complete_col, const float *partial, const float *partial_col,
                               float lr, int iters, int starts, float radius, int render_size,
                               float mask_weight, float *transform, float *history, float *best_params,
                               void *stream);

/* One step of that loop for c elements, each with its own parameters and no Adam step: genpc_pose_loss_grad_batch for clouds of
 * different sizes.  v / vert_col / partial / partial_col packed by coff / poff as above, center [c,3], params [c,10]
 *   -> loss_out [c,4] = loss, cd, |RR^T-I|_F, mask_loss;  grad [c,10]
 * with the element's own 1 / nc and 0.5 / np weights.  Refusals and return values as genpc_pose_optimize_ragged (at most 384 elements). */
int genpc_pose_loss_grad_ragged(int c, const int *coff, const int *poff, const float *v, const float *vert_col,
                                const float *center, const float *params, const float *partial,
                                const float *partial_col, float cd_weight, float reg_weight, float mask_weight,
                                float radius, int render_size, float *loss_out, float *grad, void *stream);

/* The plan of such a call (csrc/pose_ragged_plan.h; no GPU is touched): out[0] elements, [1] / [2] the largest complete / partial
 * cloud, [3] blocks per element of the transform, [4] of the Chamfer gradient, [5] blocks of the one-thread-per-element kernels,
 * [6] blocks per element of the centre's sums, [7] the Chamfer gradient rides in the silhouette gradient's launch, [8] the
 * per-pixel weights are evaluated inside the gather, [9] eight lanes per point in the gather, [10] / [11] blocks per image of the
 * per-pixel launches / of the sums, [12] the call is too large and would be refused, [13] / [14] points of the packed element
 * arrays per side (starts included), [15] the transform launch's blocks per compute unit given `cus` of them.
 * Returns 1 (c = 0: all zero); -1 with genpc_last_error set for what genpc_pose_optimize_ragged refuses before it plans. */
int genpc_pose_ragged_plan(int c, const int *coff, const int *poff, int starts, int mask, int render_size,
                           float radius, int cus, int out[16]);

/* Voxel-grid down-sampling ---------------------------------------------------- *
 * Counterpart of open3d's PointCloud.voxel_down_sample, which reg() applies to both clouds
 * before every ICP / scale search (reg_xyz.py:154-155,178-183; open3d absent, unpinned -- its
 * published definition): grid anchored at min_bound - voxel_size / 2, index =
 * floor((p - anchor) / voxel_size) in double, one output point per occupied voxel = the mean
 * of its points accumulated in point order (double).  Output order: ascending (i, j, k).
 * colors[n,3] (NULL = none): per-point colours, averaged per voxel into out_colors[n,3] the same
 * way (what open3d does for the coloured clouds of load_xyz / glb2point, utils/dataUtils.py:174-189,
 * 217-250).  voxel_size is a double, as in open3d (0.03 != 0.03f moves points near a cell face).
 * out[n,3] must hold up to n points; *out_count (device int) receives the number written, or
 * -1 when a coordinate is not finite or the grid would exceed 2^21 cells along an axis.
 * Returns -1 for voxel_size <= 0.                                                        */
int genpc_voxel_down_sample(int n, const float *xyz, const float *colors, double voxel_size,
                            float *out, float *out_colors, int *out_count, void *stream);

/* genpc_voxel_down_sample over a ragged batch: c clouds of any sizes, each with its own voxel size, one call
 * (csrc/voxel_ragged.hip).  off[c + 1] and voxel_sizes[c] are HOST arrays: cloud j is xyz[off[j] .. off[j + 1]) of the packed
 * [off[c],3] device points (colors: packed like xyz, or NULL) and is down-sampled at voxel_sizes[j].  out / out_colors have
 * off[c] rows: cloud j's voxels are written to rows off[j] .. off[j] + out_counts[j]; out_counts[c] is a DEVICE array.
 * Per cloud the rows and the count are the bits of genpc_voxel_down_sample on that cloud alone: the grid anchored at the
 * cloud's OWN min_bound - voxel / 2, ascending (i, j, k), means in double in ascending point index.  out_counts[j] = -1 when
 * a coordinate of cloud j is not finite or its grid exceeds 2^21 cells on an axis (its rows are then unspecified, every other
 * cloud is unaffected); an empty cloud gives 0.
 * Asynchronous on `stream`: a fixed number of launches whatever c is (bounds, keys, two stable radix sorts -- by key, then by
 * cloud number --, run heads, one scan, means and counts, the error fold); the offsets and sizes travel by value in the kernel
 * arguments, so nothing of the host arrays is read after return and no copy is enqueued -- which bounds c.
 * Returns 1 on success (also for c == 0: nothing written), 0 on a HIP error; -1 with genpc_last_error set
 * ("genpc_voxel_down_sample_ragged: ...") and nothing enqueued for c < 0, c > GENPC_VOXEL_RAGGED_MAX_CLOUDS, a null table,
 * off[0] != 0, descending offsets, more than 2^28 points, a voxel size that is not > 0 (the message names the cloud), or a
 * null device pointer with work to do.                                                                                  */
#define GENPC_VOXEL_RAGGED_MAX_CLOUDS 256
int genpc_voxel_down_sample_ragged(int c, const int *off, const float *xyz, const float *colors,
                                   const double *voxel_sizes, float *out, float *out_colors,
                                   int *out_counts, void *stream);

/* ICP + scale search --------------------------------------------------------- *
 * Batched point-to-point ICP with the semantics of open3d's registration_icp as
 * reg_xyz.py calls it (:18-20,28-37: TransformationEstimationPointToPoint, default
 * criteria 30 iterations / 1e-6 / 1e-6): K candidates share source[ns,3] and
 * target[nt,3] and differ in their initial transform init[K,16] (row-major 4x4,
 * DOUBLE, device memory).  out_T[K,16] double, stats[K,3] double = fitness,
 * inlier_rmse, iterations.  Correspondence: fp32 nearest neighbour with
 * d2 <= max_dist^2.                                                            */
int genpc_icp_batch(int k, int ns, const float *source, int nt, const float *target,
                    double max_dist, const double *init, int max_iter,
                    double rel_fitness, double rel_rmse, double *out_T,
                    double *stats, void *stream);

/* Which implementation genpc_icp_batch runs for nt targets (csrc/icp_plan.h; no GPU is touched):
 * out[0] = 1 the one-workgroup solve (one launch, target grid in LDS), 0 the multi-launch loop
 * (five launches per pass); out[1] = the grid's cell budget (8192, 4096, 2048 or 1024; 0 for the
 * loop); out[2] = the launch's dynamic LDS in bytes (0 for the loop).  Returns -1 for out == NULL. */
int genpc_icp_plan(int nt, int out[3]);

/* genpc_icp_batch over a ragged batch: c (source, target) pairs of any sizes, each with its own candidates, one call.
 * soff / toff / koff [c + 1] are HOST arrays (by value in the kernel arguments: nothing is read after return, which bounds c):
 * pair j is source[soff[j] .. soff[j + 1]) against target[toff[j] .. toff[j + 1]) of the packed device clouds, its candidates
 * are the rows koff[j] .. koff[j + 1] of init[K,16] (K = koff[c]; row-major 4x4, DOUBLE, device); out_T[K,16] and stats[K,3]
 * as in genpc_icp_batch.  The pairs whose target count gets the one-workgroup plan (genpc_icp_plan) are ALL solved by one
 * launch, a workgroup per (pair, candidate) with its own pair's cell budget: each of their candidates gets the BITS of
 * genpc_icp_batch on that pair alone, in both arithmetic modes.  The others run, one pair after the other inside the call,
 * through genpc_icp_batch's multi-launch loop and get what it gives them.  A pair without candidates is skipped.
 * Returns 1 on success (also when there is no candidate: nothing written), 0 on a HIP error; -1 with genpc_last_error set
 * ("genpc_icp_batch_ragged: ...") and nothing enqueued for c < 0, max_iter < 0, c > GENPC_ICP_RAGGED_MAX_PAIRS, a null table,
 * a table that does not start at 0 or descends, more than 2^28 points on a side, more than 2^20 candidates, a pair that has
 * candidates and an empty source or target (the message names it), or a null device pointer with work to do.            */
#define GENPC_ICP_RAGGED_MAX_PAIRS 256
int genpc_icp_batch_ragged(int c, const int *soff, const int *toff, const int *koff,
                           const float *source, const float *target, double max_dist,
                           const double *init, int max_iter, double rel_fitness, double rel_rmse,
                           double *out_T, double *stats, void *stream);

/* How a genpc_icp_batch_ragged call with these target offsets is split (csrc/icp_ragged_plan.h; no GPU is touched):
 * out[0] = the pairs solved by the one launch, out[1] = the pairs sent to the multi-launch loop (a pair without targets is
 * on neither side), out[2] = the launch's dynamic LDS in bytes, the largest of its pairs' genpc_icp_plan.  Returns 1; -1
 * with genpc_last_error set for out == NULL, c < 0, c > GENPC_ICP_RAGGED_MAX_PAIRS, a null or ill-formed toff.          */
int genpc_icp_ragged_plan(int c, const int *toff, int out[3]);

/* Scores of iterative_scale_search (reg_xyz.py:60-96) for K anisotropic scale
 * candidates scales[K,3] in one batched NN launch:
 *   scores[k] = mean sqrt(NN(source*scales[k] -> target))
 *             + cd_inv_weight * mean sqrt(NN(target -> source*scales[k])).    */
int genpc_scale_search_scores(int k, int ns, const float *source, int nt,
                              const float *target, const float *scales,
                              float cd_inv_weight, float *scores, void *stream);

/* genpc_scale_search_scores over a ragged batch: c (source, target) pairs of any sizes, each with its own candidates, one call.
 * soff / toff / koff [c + 1] are HOST arrays (by value in the kernel arguments: nothing is read after return, which bounds c):
 * pair j is source[soff[j] .. soff[j + 1]) against target[toff[j] .. toff[j + 1]) of the packed device clouds, its candidates
 * are the rows koff[j] .. koff[j + 1] of scales[K,3] (K = koff[c]; float32, device); scores[K] is device float32:
 *   scores[k] = float(mean64 sqrtf(NN(s_k o source -> target))) + float(mean64 sqrtf(NN(target -> s_k o source))) * cd_inv_weight
 * with s_k o p = (float)((double)p * (double)s) per axis.  Two launches whatever c and K are: one grid per pair's target, then
 * one workgroup per candidate, which keeps the scaled source and its own grid in LDS and adds the distances where it finds
 * them; no copy of either cloud and no distance array is written, no floating-point atomic is used.
 * On finite input every candidate's score is the BITS of genpc_scale_search_scores on its pair alone, in both arithmetic
 * modes, wherever the pair stands in the batch.  A pair whose source does not fit a compute unit's LDS
 * (genpc_scale_search_ragged_plan) is scored inside the call by genpc_scale_search_scores on its slices.  A pair without
 * candidates is skipped.  Not finite: a pair whose target holds a non-finite coordinate gets NaN for all its scores, a
 * candidate whose scaled source holds one (a non-finite scale, a product that overflows) gets NaN, the others do not notice
 * (for the pairs of the one launch; what genpc_scale_search_scores returns on such input is not defined).
 * Returns 1 on success (also when there is no candidate: nothing written), 0 on a HIP error; -1 with genpc_last_error set
 * ("genpc_scale_search_scores_ragged: ...") and nothing enqueued for c < 0, c > GENPC_SCALE_SEARCH_RAGGED_MAX_PAIRS, a null
 * table, a table that does not start at 0 or descends, more than 2^28 points on a side, more than 2^20 candidates, a pair that
 * has candidates and an empty source or target (the message names it), or a null device pointer with work to do.        */
#define GENPC_SCALE_SEARCH_RAGGED_MAX_PAIRS 256
int genpc_scale_search_scores_ragged(int c, const int *soff, const int *toff, const int *koff,
                                     const float *source, const float *target, const float *scales,
                                     float cd_inv_weight, float *scores, void *stream);

/* How a genpc_scale_search_scores_ragged call with these source offsets is split (csrc/scale_search_ragged_plan.h; no GPU is
 * touched): out[0] = the pairs scored by the one launch, out[1] = the pairs sent to genpc_scale_search_scores (a pair without
 * source points is on neither side), out[2] = the launch's dynamic LDS in bytes, the largest of its pairs'.  Returns 1; -1
 * with genpc_last_error set for out == NULL, c < 0, c > GENPC_SCALE_SEARCH_RAGGED_MAX_PAIRS, a null or ill-formed soff. */
int genpc_scale_search_ragged_plan(int c, const int *soff, int out[3]);

/* Hardware-premise probe ------------------------------------------------------ *
 * D[p] = A[p] B[p] + C[p] for `problems` independent 32x16 * 16x32 + 32x32 products computed by ONE
 * v_mfma_f32_32x32x16_f16 each (A, B: f16 bit patterns, row-major; C, D float32; device memory).
 * The default nearest-neighbour filter's proof leans on this instruction's internal summation error
 * being <= 6.5 * 2^-24 * sum|terms| (csrc/nn_f16.hip); tests/test_gpu_mfma_premise.py measures it
 * with this entry on the box the suite runs on.                                                  */
int genpc_mfma_f16_probe(int problems, const unsigned short *a, const unsigned short *b,
                         const float *c, float *d, void *stream);

/* out[i] = decode(encode(base[i], v[i])) of the 16-bit lower-bound code the nearest-neighbour filter hands its second and
 * third list minima to the finish step in (csrc/nn.h: list_enc / list_dec).  For v >= base the result must never exceed
 * v (tests/test_gpu_fastdiv.py::test_list_codes_are_lower_bounds).  Device memory, n elements.               */
int genpc_list_code_probe(long long n, const float *base, const float *v, float *out, void *stream);

/* fast[i] = csrc/fastdiv.h's shared-reciprocal division num[i] / den[i] (scalar form), fast_packed[i] = its packed
 * form, ieee[i] = the compiler's correctly rounded division, in_range[i] = 1 where the callers' range test
 * (both magnitudes in [2^-50, 2^50]) lets the fast form be used: there the three must agree bit for bit
 * (tests/test_gpu_fastdiv.py).  All arrays device memory, n elements.                              */
int genpc_fastdiv_probe(long long n, const float *num, const float *den, float *fast,
                        float *fast_packed, float *ieee, unsigned char *in_range, void *stream);

/* Grid probes: csrc/grid.h's cell function, sizing, skip bound and cell range and csrc/grid.hip's two builds, run on the
 * caller's inputs; the kernels behind them call those helpers themselves (tests/test_gpu_grid.py).  Device memory unless noted.
 * A header is 13 words: lo[3], inv, h, slack[3] (float32), g[3], cells, bad (int32); a frame is its first 11.
 *
 * genpc_grid_build_probe, moff == null: the build of b clouds xyz[b][n][3] for cells_target and 1 <= cells_max <= 15360 cells:
 * hdr[b], start[b][cells_max + 1], sorted[b][n][4] (x, y, z, bits of the index), pos_of[b][n] and orig_of[b][n] (either may be
 * null).  moff != null (HOST, b + 1 offsets; noff likewise, null: moff): the ragged build of b clouds packed in xyz, each
 * sized for itself; cloud j's cell table starts at start[moff[j] + 65 j], its points at sorted[moff[j]] with the index inside
 * the cloud; a cloud with noff[j + 1] == noff[j] is not built and its pieces are not written; n, cells_*, pos_of, orig_of are
 * not used.  Returns 0 when no cloud has a query.                                                         */
int genpc_grid_build_probe(int b, int n, const float *xyz, const int *noff, const int *moff, int cells_target,
                           int cells_max, void *hdr, int *start, float *sorted, int *pos_of, int *orig_of, void *stream);

/* frames[i] = grid_size<16, false> (coarse == 0: the builds above) or grid_size<12, true> (nn_grid.hip's 4 x 4 x 4 numbering) of
 * the box mn[i][3] .. mx[i][3] for cells_target[i], cells_max[i]; one thread per box.                            */
int genpc_grid_size_probe(int nbox, int coarse, const float *mn, const float *mx, const int *cells_target,
                          const int *cells_max, void *frames, void *stream);

/* For one header, queries q[nq][3] and points p[n][3]: qcell[nq][3], pcell[n][3] = grid_cell1 per axis; qslack[nq][3] =
 * grid_slack; per pair (j, i), at [j n + i]: gap1[..][3], gap4[..][3] = grid_gap per axis of the point's cell and of its aligned
 * block of four cells; bound[..][3] = fma(gx,gx,fma(gy,gy,gz*gz)) * kGridShrink of gap1, fma(gy,gy,gz*gz) * kGridShrink of gap1,
 * the first form of gap4; sq[..][2] = sqdist<0>, sqdist<1> of p - q.  slab[nq][3][gmax][2], for c < g of the axis: grid_gap(0, c)
 * and grid_gap(c, g - c) of the shell walk; slab_bound the same shape: (m * m) * kGridShrink.  mn[3], mx[3] (both or neither):
 * outer walls of the border cells, as icp.hip passes them.                                                 */
int genpc_grid_bound_probe(const void *hdr, int nq, const float *q, int n, const float *p, const float *mn,
                           const float *mx, int gmax, int *qcell, int *pcell, float *qslack, float *gap1, float *gap4,
                           float *bound, float *sq, float *slab, float *slab_bound, void *stream);

/* range[nq][3][2] = grid_cell_range of q[nq][3] with radius[nq][3] on each axis: the cells that can hold a point within the
 * radius; clip[nq][3][2] != null: grid_cell_range_in, the range clipped to [clip[..][0], clip[..][1]].                */
int genpc_grid_range_probe(const void *hdr, int nq, const float *q, const float *radius, const int *clip, int *range,
                           void *stream);

/* Silhouette backward probe: everything mask_step does after its splat, on the caller's image (tests/test_gpu_mask_backward_probe.py).
 * planes[5, P], P = S * S: the five planes as the splat leaves them for `blend` (0: T, D, N_r, N_g, N_b; 1: m, D', N'_r, N'_g, N'_b);
 * ref_img[P, 3] the reference image; pts[n, 3] with colours col[n, 3] (null: white), center[3], params[10]; radius is the
 * radius the planes were drawn with and is used as given (no factor 1.1).  Runs mask_ref_kernel on ref_img, the image sums of the
 * planes, then mask_sums_kernel, mask_w_kernel (fuse_w == 0) and mask_grad_kernel<sub8 ? 8 : 1, blend, fuse_w> as one image with
 * genpc_mask_loss's grids.  accum_out[16] (double): 0..12 the gradient sums of mask_grad_kernel (d / d R row-major, d / d log-scale
 * at 9 without its factor s, d / d t at 10..12), 15 mask_weight * loss.  fuse_w == 0: W1_out[P], W4_out[P, 4] (either may be null)
 * receive the per-pixel weights.  Device memory.  Returns 1 / 0 / -1 (S < 2, n < 1, a null input).                      */
int genpc_mask_backward_probe(int S, int blend, int sub8, int fuse_w, const float *planes, const float *ref_img, int n,
                              const float *pts, const float *col, const float *center, const float *params, float radius,
                              float mask_weight, double *accum_out, float *W1_out, float *W4_out, void *stream);

/* Sampling-check probe: the device-side check every farthest point sampling gets (csrc/fps_verify.hip: fps_verify_kernel and the
 * poisoning kernel behind it, in line, in the call's arithmetic mode) run on the caller's arrays (tests/test_gpu_fps_check.py).
 * 1 <= nj <= 8 clouds in one job table; n, k and the three pointer tables are HOST arrays, xyz[q][n_q][3], out[q][k_q] (the
 * sequence) and pdist[q][k_q] (the running minimum of every sample when it was drawn; [0] is not read) device memory.  The verdict
 * is what a caller of genpc_fps sees: out[q][0] stays 0, becomes -2 (a step is wrong), or stays -1 if it was -1.  nseg == 0: the
 * sample lists are cut into as many segments as in production (csrc/fps_plan.h: fps_verify_segments); 1 <= nseg <= 16 forces
 * that number.  single != 0: as for the large sampler's clouds (never cut, unless nseg forces it).  Returns 1 / 0; -1 with
 * genpc_last_error set for nj outside 1..8, a null pointer, k_q < 1, k_q > n_q, nseg outside 0..16, more than 4194304 points in all. */
int genpc_fps_verify_probe(int nj, const int *n, const int *k, const float *const *xyz, int *const *out,
                           const float *const *pdist, int nseg, int single, void *stream);

/* Farthest point sampling --------------------------------------------------- *
 * Deterministic counterpart of fpsample.fps_sampling as the reference uses it
 * (main.py:21-24, reg_xyz.py:215, DepthPrompting.py:88; third-party, random start):
 * start index 0, fp32 squared distances in the library's arithmetic mode, first
 * arg-max.  xyz[C,N,3] -> out_idx[C,k] int32, C clouds side by side.  Returns -1
 * unless 0 < k <= n <= 4194304.  Three samplers return the same sequences, and a
 * cloud's point count decides which it takes (csrc/fps_plan.h, genpc_fps_plan):
 * up to 24576 points one workgroup with its running minima in LDS, up to 262144
 * the multi-workgroup kernel, beyond that one workgroup with its state in global
 * memory (csrc/fps_large.hip).  out_idx[c][0] is 0 for a good sequence; -1: the
 * hand-off among the cloud's workgroups timed out (something kept them from running
 * together; only the multi-workgroup kernel has one) or a one-workgroup sampler
 * exhausted its bound of sweeps; -2: the finished sequence failed the device-side
 * check of every step against the definition -- sample that cloud again
 * (genpc_amd/fps.py does).                                                       */
int genpc_fps(int c, int n, const float *xyz, int k, int *out_idx, void *stream);

/* The same for C clouds of DIFFERENT sizes in one pass (the metric's two subsamplings and the fused
 * cloud's run side by side: a step costs its latency, not its work): host arrays n[C], k[C],
 * xyz[C] (device pointers to [n_j,3]), out_idx[C] (device pointers to [k_j]).  The clouds of one
 * call may take different samplers.                                                              */
int genpc_fps_multi(int c, const int *n, const int *k, const float *const *xyz,
                    int *const *out_idx, void *stream);
/* genpc_fps_multi with EVERY cloud on the sampler of csrc/fps_large.hip, for any 0 < k <= n <= 4194304 (one workgroup per
 * cloud, no hand-off, nothing that has to be co-resident; its check is always in line).  Same contract, same sequences.  */
int genpc_fps_large(int c, const int *n, const int *k, const float *const *xyz,
                    int *const *out_idx, void *stream);
/* Which sampler a cloud of n points takes, and what the large sampler needs for it (csrc/fps_plan.h; no GPU work):
 * out[0] sampler (0 one workgroup / LDS -- genpc_fps_tune(256) sends such a cloud to 1 --, 1 multi-workgroup, 2 large; -1 refused),
 * and for the large sampler, else 0: out[1] cells of its grid at most, out[2] cells asked for, out[3] running minima and sorted
 * points (n padded), out[4] chunk maxima, out[5] cell table entries, out[6] LDS bytes, out[7] 0 = the grid is built by the shared
 * multi-workgroup build.  force_large != 0: as genpc_fps_large plans it.  Returns 1, or -1 when the cloud is refused or out is null. */
int genpc_fps_plan(int n, int force_large, int out[8]);
/* The device-side check of finished sequences OFF the caller's critical path (calling host thread; returns the previous
 * setting).  1: samplings of clouds the one-workgroup kernel takes (<= 24576 points) return without waiting for their check --
 * the cloud, the indices and the recorded minima are copied (stream-ordered) and checked on a side stream of the library's own;
 * a failed check is counted instead of poisoning out_idx[c][0].  genpc_fps_deferred_check(stream) waits for the checks of the
 * samplings enqueued on `stream` by this device so far and returns how many failed since the last call (-1: error): when it is
 * not 0 the caller samples again with the check in line (genpc_fps_defer(0)).  genpc_amd/pipeline.py does so once per
 * completed scan.  0 (default): out_idx is final when the call's work on the stream is.  (2: test hook -- deferred, and the
 * check's copy of one recorded minimum is zeroed: the check must fail, tests/test_gpu_fps.py.)                                */
int genpc_fps_defer(int on);
/* Makes the side streams the library pairs with `stream` (alignment loop, sampling check) and gives each a first command: a
 * stream's hardware queue is decided when it is first used, and the pairing overlaps best when these come before other
 * streams of the process (csrc/pose.hip pose_side_of).  Optional; pipeline.run_in_lanes calls it before making its lanes.  Returns 1. */
int genpc_streams_prepare(void *stream);
int genpc_fps_deferred_check(void *stream);
/* Test hook (calling host thread; returns the previous setting): 256 = every cloud of genpc_fps* takes the multi-workgroup
 * kernel, never the one-workgroup kernel with spatial pruning (tests compare the two); 0 = the default choice.  Any other
 * value returns -1 and sets genpc_last_error. */
int genpc_fps_tune(int mode);
/* Diagnostics: rounds[j] (host, c <= 32) = inter-workgroup exchanges cloud j of the last
 * genpc_fps_multi / genpc_fps_large call on this stream took (one exchange yields several samples; for the
 * one-workgroup samplers: the rounds of candidates).  Synchronises.  */
int genpc_fps_stats(int c, int *rounds, void *stream);

/* Statistical outlier filter ------------------------------------------------ *
 * mean_out[N] = mean Euclidean distance of every point to its k nearest points of
 * the same cloud, itself included (the per-point statistic of open3d's
 * remove_statistical_outlier, utils/dataUtils.py:648-662 -> reg_xyz.py:134,217).
 * k in {8, 16, 20, 32}; -1 otherwise.  NaN and infinite distances are never among the
 * k: a point with a non-finite coordinate gets 0 / 0 = NaN, every other point the mean
 * it has without those points.                                                   */
int genpc_knn_mean_distance(int n, const float *xyz, int k, float *mean_out,
                            void *stream);

/* Ragged form: c clouds of any sizes in one call.  Cloud j is xyz[off[j] .. off[j+1]); off: a HOST array of c + 1 ascending
 * ints, off[0] = 0, copied before the call returns (it travels in the kernel arguments); xyz [off[c],3]: fp32, device, packed
 * in cloud order; k in {8, 16, 20, 32}.  mean_out[off[j] + i] holds the bits of genpc_knn_mean_distance(n_j, xyz + 3 off[j],
 * k, ..)[i] on cloud j alone, in the call's arithmetic mode, NaN for NaN; a non-finite coordinate affects its own cloud only.
 * An empty cloud is allowed and gets no work and no word of mean_out.
 * Asynchronous on `stream`: two launches whatever c is (the ragged grid build, the search), scratch from the library's
 * workspace, no copy, no host read-back, no synchronisation (csrc/knn.hip).  Returns 1 on success; -1 with genpc_last_error
 * set, nothing enqueued and nothing written for c < 0, c > 384, a null off, off[0] != 0, descending offsets,
 * off[c] > 2^28, a k outside the set, or (when there is work) a null xyz or mean_out; 1 at once with nothing enqueued
 * if c == 0 or off[c] == 0.                                                                                            */
int genpc_knn_mean_distance_ragged(int c, const int *off, const float *xyz, int k, float *mean_out,
                                   void *stream);

/* The whole statistical outlier filter for c clouds in one call (open3d's remove_statistical_outlier per cloud): clouds, off
 * and k as above.  With m_i = (double) of cloud j's i-th mean and n its point count, every operation a separately rounded
 * fp64 operation and NOTHING fused:
 *   S(v)   the sum of n fp64 values in this order and no other: 1024 partial sums p[t], each starting at +0.0; p[t] adds
 *          the elements i = t, t + 1024, t + 2048, ... in ascending i; then for w = 512, 256, ..., 1: p[t] = p[t] + p[t + w]
 *          for t < w; S = p[0].  A function of n alone: not of c, of the cloud's place in the batch or of the launch shape;
 *          no floating-point atomic.
 *   mean = S(m) / n;   std = sqrt(S((m_i - mean) * (m_i - mean)) / (n - 1));   thr = mean + std_ratio * std
 *   keep[off[j] + i] = m_i < thr ? 1 : 0;   kept[j] = the number of ones;   stats[j] = (mean, std, thr)
 * So a one-point cloud has std = 0 / 0 = NaN and keeps nothing, a cloud with a NaN mean keeps nothing, and an empty cloud
 * gets stats (NaN, NaN, NaN) and kept 0.  mean_out [off[c]] (fp32; null: the means stay in the workspace), stats [c,3]
 * (fp64) and kept [c] (int32) may be null; keep [off[c]] (bytes) is required.  Every word of keep, stats and kept that belongs
 * to the call is written.
 * Asynchronous on `stream`: three launches whatever c is (the ragged grid build, the search, one workgroup per cloud for the
 * statistics and the mask; no kernel spins or waits on another workgroup), scratch from the library's workspace, no copy,
 * no host read-back, no synchronisation (csrc/knn.hip).  Returns as genpc_knn_mean_distance_ragged does; the null pointers
 * refused are xyz and keep.                                                                                             */
int genpc_outlier_filter_ragged(int c, const int *off, const float *xyz, int k, double std_ratio,
                                float *mean_out, double *stats, unsigned char *keep, int *kept,
                                void *stream);

/* k nearest neighbours ------------------------------------------------------- *
 * For every query of xyz[B,NQ,3] its k nearest targets of xyz2[B,NT,3], 1 <= k <= 32: dist[B,NQ,k] (squared distances)
 * and idx[B,NQ,k] (what the reference asks of scipy's KDTree.query in linear_interpolation, utils/dataUtils.py:128-134,
 * with k = 2 or 5).  Order: that of the 64-bit key distance bits << 32 | target index -- distances ascend, among
 * bit-equal distances the lower index comes first, and the same order decides which of several equal candidates holds
 * the k-th place.  The distance is the library's (arithmetic mode of the call): column 0 holds the bits of
 * genpc_nm_distance on finite input.  Only targets at a distance < +inf are listed (a NaN or infinite distance never
 * enters); the slots past the listed ones -- NT < k, non-finite input -- hold (+inf, -1).  Every output word is written.
 * Exact: a pruned search on the uniform grid (csrc/knn_query.hip).  Returns -1 and writes nothing for k < 1, k > 32 or
 * NT < 1 with NQ > 0; 1 at once for NQ == 0 or B == 0.                                                                */
int genpc_knn_query(int b, int nq, const float *xyz, int nt, const float *xyz2, int k,
                    float *dist, int *idx, void *stream);

/* Ragged form: c independent (queries, targets) pairs of any sizes in one call.  Pair j has the queries xyz[noff[j] .. noff[j+1])
 * and the targets xyz2[moff[j] .. moff[j+1]); noff, moff: HOST arrays of c + 1 ascending ints, noff[0] = moff[0] = 0, copied
 * before the call returns (the table travels in the kernel arguments); xyz [noff[c],3], xyz2 [moff[c],3]: fp32, device, packed
 * in pair order (as for genpc_nm_distance_ragged); 1 <= k <= 32.  dist [noff[c],k] (fp32 squared distances) and idx [noff[c],k]
 * (int32, counted INSIDE the pair's own target cloud) are packed in pair order: pair j's rows are bit for bit what
 * genpc_knn_query(1, N_j, xyz + 3 noff[j], M_j, xyz2 + 3 moff[j], k, ..) returns for that pair alone, in the call's arithmetic
 * mode -- the same key order distance bits << 32 | index, the same rule for the k-th place, the same non-finite rules: only
 * targets at d < +inf are listed, the slots past them hold (+inf, -1), a target cloud with a non-finite coordinate is searched
 * without culling.  M_j < k is legal and fills the tail with (+inf, -1).  A pair's non-finite input affects that pair only.
 * Every output word that belongs to a pair with queries is written; a pair with N_j == 0 writes nothing and its targets, if
 * any, are not looked at.  The result does not depend on where a pair stands in the call or on the other pairs: every pair's
 * targets get a grid of their own, sized otherwise than the single call's, and the search is exact on any grid.
 * Asynchronous on `stream`: three launches whatever c is (the ragged grid build, one workgroup per pair ordering its queries,
 * the search; no kernel spins or waits on another workgroup), scratch from the library's workspace, no copy, no host
 * read-back, no synchronisation (csrc/knn_query.hip).  Returns 1 on success; 1 at once with nothing enqueued if c == 0 or
 * noff[c] == 0 (after the offsets have been checked); -1 with genpc_last_error set, nothing enqueued and nothing written for
 * k < 1, k > 32, c < 0, c > 384, a null table, offsets that do not start at 0 or descend, more than 2^28 points on a side, a
 * pair with queries and no targets, or (when there is work) a null xyz, xyz2, dist or idx; 0 on a HIP error.             */
int genpc_knn_query_ragged(int c, const int *noff, const float *xyz, const int *moff, const float *xyz2, int k,
                           float *dist, int *idx, void *stream);

/* Directed Hausdorff distance (UHD) ------------------------------------------ *
 * From the queries xyz[B,N,3] to the targets xyz2[B,M,3] (fp32, device), exact in fp64: the coordinates are widened and
 * every pair's s = ((dx*dx) + (dy*dy)) + (dz*dz), d = query - target, is evaluated in fp64 in that order with no fused
 * multiply-add -- scipy's cdist(.., 'euclidean') before its sqrt, which is what the reference's UHD (metric.py:105-132)
 * takes min over axis 1 and max of.  out_d2[B] (fp64) = max_i min_j s_ij: sqrt is monotone, so sqrt(out_d2) has the bits
 * of the reference's hd.  out_ij[B,2] = the witness (i*, j*): i* the lowest query index that attains the maximum, j* the
 * lowest target index that attains query i*'s minimum, both judged on the fp64 s (numpy's argmax / argmin).
 * Non-finite coordinates: a pair whose s is NaN is skipped (the minimum is IEEE minNum), a query all of whose pairs are
 * NaN has the minimum +inf; so out_d2 is never NaN, it is +inf if any query has no finite pair or an infinite minimum,
 * i* is always a valid query index, and j* is -1 when no target of i* attains its minimum (every pair NaN).  numpy
 * returns NaN there; finite input is the contract.
 * Asynchronous on `stream`, scratch from the library's workspace, no host read-back (csrc/uhd.hip).  Returns 0 on success;
 * 1 with nothing written if B == 0; -1 with genpc_last_error set and nothing written if N <= 0, M <= 0, a pointer is
 * null, or the problem is too large for one launch (B > 65535, N > 2^30, M > 65535 * 512).                            */
int genpc_uhd(int b, int n, const float *xyz, int m, const float *xyz2,
              double *out_d2, int *out_ij, void *stream);

/* Ragged UHD: c independent (queries, targets) pairs of any sizes in one call.  Pair j has the queries xyz[noff[j] .. noff[j+1])
 * and the targets xyz2[moff[j] .. moff[j+1]); noff, moff: HOST arrays of c + 1 ascending ints, noff[0] = moff[0] = 0, copied
 * before the call returns; xyz [noff[c],3], xyz2 [moff[c],3]: fp32, device, packed in pair order (as for
 * genpc_nm_distance_ragged).  out_d2[j] (fp64) = max over pair j's queries of the minimum over its targets of
 * s = ((dx*dx) + (dy*dy)) + (dz*dz), d = query - target, in fp64 on the widened coordinates, in that order, nothing fused:
 * the bits of genpc_uhd(1, N_j, .., M_j, ..) on that pair alone.  out_ij[j] = (i*, j*), counted inside the pair's own slices:
 * i* the lowest query that attains the maximum, j* the lowest target of the pair with s == out_d2[j] for query i*, or -1 if
 * none has (on finite input that is genpc_uhd's witness).
 * Non-finite coordinates, as for genpc_uhd: a pair of points whose s is NaN is skipped (the minimum is IEEE minNum), a query
 * all of whose s are NaN has the minimum +inf; so out_d2 is never NaN, it is +inf where a query has no finite pair or an
 * infinite minimum, i* is always a valid query index, and j* follows the rule above (the lowest target at s == +inf, -1 if
 * every s of query i* is NaN).  One pair's non-finite input affects that pair only.  Finite input is the contract.
 * The same bits on every run: the minima are folded with integer atomics on the bit pattern, no floating-point atomic.
 * Asynchronous on `stream`: four launches whatever c is, the pair table in the kernel arguments, scratch from the library's
 * workspace (8 bytes a query), no copy, no host read-back, no synchronisation (csrc/uhd_ragged.hip).  Returns 0 on success;
 * 1 with nothing written if c == 0; -1 with genpc_last_error set, nothing enqueued and nothing written for c < 0, c > 384,
 * null noff / moff, noff[0] != 0 or moff[0] != 0, descending offsets, noff[c] or moff[c] > 2^28, a pair with no queries or
 * no targets (one empty on both sides too: the maximum or minimum of an empty set is undefined), a null device pointer, or
 * a pair too large for one launch: every pair's M_j <= 65535 * 512 = 33553920 targets.                                 */
int genpc_uhd_ragged(int c, const int *noff, const float *xyz, const int *moff, const float *xyz2,
                     double *out_d2, int *out_ij, void *stream);

/* Surface samples of a triangle mesh ----------------------------------------- *
 * count area-weighted samples of the mesh vertices[nv,3] (fp32) / faces[nf,3] (int32), uniform inside a face: the published
 * algorithm of trimesh.sample.sample_surface (what glb2point draws its clouds with, utils/dataUtils.py:217-250), with this
 * library's own random numbers and INTEGER face weights, so that every bit of sample i follows from (mesh, seed, i) alone --
 * not from count, the launch shape or the order of a parallel sum.  The definition:
 *   areas    face f with vertices v0, v1, v2 widened to fp64: e1 = v1 - v0, e2 = v2 - v0, c = e1 x e2 with every component
 *            (a*b) - (c*d) = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x), nothing fused,
 *            s = ((cx*cx) + (cy*cy)) + (cz*cz), A_f = sqrt(s) correctly rounded (twice the area: the factor cancels).
 *   weights  Amax = max_f A_f, e = ilogb(Amax), w_f = (uint64) floor(ldexp(A_f, 38 - e)): the largest face weighs
 *            [2^38, 2^39), a face 2^38 times smaller than the largest -- a degenerate one too -- weighs 0 and is never
 *            drawn.  cum[f] = sum_{g <= f} w_g in uint64 and W = cum[nf - 1] < 2^63.
 *   words    (x0, x1, x2, x3) = Philox4x32-10 with counter (i & 0xffffffff, i >> 32, 0, 0) and key
 *            (seed & 0xffffffff, seed >> 32); multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85.
 *   face     t = the high 64 bits of (x0 | x1 << 32) * W; the face is the first f with cum[f] > t
 *            (numpy's searchsorted(cum, t, side="right")).
 *   place    r1 = (x2 >> 8) * 2^-24, r2 = (x3 >> 8) * 2^-24 in fp32; if r1 + r2 > 1 (the fp32 sum) both are replaced by
 *            1 - r (exact); b0 = (1 - r1) - r2.  (The one fp32 sum that rounds, 1 + 2^-24 -> 1, is not folded and gives
 *            b0 = -2^-24: once in 2^24 samples a point lies that far, in units of an edge, outside its face.)
 *   point    per component in fp64 (v0 + (e1*r1)) + (e2*r2), rounded once to fp32  -> out_xyz[count,3].
 *   colour   with vertex_colors[nv,3]: ((c0*b0) + (c1*r1)) + (c2*r2) in fp64, rounded to fp32, then x < 0 -> 0, x > 1 -> 1
 *            -> out_colors[count,3].  The barycentric weights ARE (b0, r1, r2): nothing is solved for.
 * out_face[count] (the drawn face) and out_bary[count,3] = (b0, r1, r2) are optional (NULL), as are the colours.
 * *out_status (device int): 1 when done; -1 if a face has an index outside [0, nv) (checked before anything is loaded
 * through it), if a vertex of a face is not finite (a vertex no face uses may be anything), or if every weight is 0.
 * With -1 the outputs are unspecified, but every word of them is written and nothing is read or written out of range.
 * workspace: genpc_mesh_sample_bytes(nf) bytes of device memory (-1: nf outside [1, 2^24]), the caller's.  After the call
 * it holds, at byte 256, uint64 local[nf] -- cum restarted every 1024 faces (local[f] = cum[f] - cum[1024*(f/1024) - 1]) --
 * and, at byte 256 + 8 nf rounded up to a multiple of 256, uint64 chunk[ceil(nf / 1024)] = cum[min(1024 (k+1), nf) - 1].
 * Asynchronous on `stream`: a memset and four launches, no host read-back (csrc/mesh_sample.hip).  Returns 1; -1 with
 * genpc_last_error set and nothing enqueued for nf < 1, nf > 2^24, count < 1, nv < 1, out_colors without vertex_colors or
 * a null required pointer.                                                                                            */
int genpc_mesh_sample_bytes(int nf);
int genpc_mesh_sample(int nv, const float *vertices, const float *vertex_colors, int nf,
                      const int *faces, int count, unsigned long long seed, float *out_xyz,
                      float *out_colors, int *out_face, float *out_bary, int *out_status,
                      void *workspace, void *stream);

/* Ragged surface sampling: c meshes of any sizes in one call, each with its own seed and sample count.  Mesh j has the vertices
 * vertices[voff[j] .. voff[j+1]) (and vertex_colors, packed the same way, optional), the faces faces[foff[j] .. foff[j+1]) --
 * int32 indices counted inside the mesh's OWN vertices -- and the output rows [soff[j] .. soff[j+1]); voff, foff, soff: HOST
 * arrays of c + 1 ascending ints starting at 0, seeds: a HOST array of c words; all four are copied before the call returns.
 * Mesh j's rows of out_xyz [soff[c],3] and of the optional out_colors [soff[c],3], out_face [soff[c]] (an index inside the
 * mesh's own faces) and out_bary [soff[c],3] are the bits of genpc_mesh_sample on that mesh alone with count = soff[j+1] -
 * soff[j] and seed = seeds[j]: the definition above holds per mesh -- Amax, the weight shift and the cumulative weights are the
 * mesh's own, sample i of a mesh uses Philox counter i (the index inside the mesh) and key seeds[j] -- and so does the prefix
 * property: a sample does not depend on its mesh's count, on the other meshes or on the mesh's place in the batch.
 * out_status[j] (device ints, c of them): 1 or -1 by genpc_mesh_sample's rules judged on mesh j alone; a face index >= nv_j is
 * bad even where the packed array has a vertex there, and is checked before anything is loaded through it.  A mesh with -1
 * has every word of its outputs written as the single call writes them and changes no bit of any other mesh.  A count of 0
 * is allowed: the mesh's status is still written.
 * Asynchronous on `stream`: a memset and FOUR launches whatever c is, the tables in the kernel arguments, scratch from the
 * library's workspace (16 bytes a mesh, 8 bytes a face, 8 bytes per chunk of 1024 faces and per mesh), integer atomics only
 * (the same bits on every run), no copy, no host read-back, no synchronisation (csrc/mesh_sample_ragged.hip).  Returns 1 (c == 0
 * too, with nothing done); -1 with genpc_last_error set ("genpc_mesh_sample_ragged: ...") and nothing enqueued for c < 0,
 * c > GENPC_MESH_SAMPLE_RAGGED_MAX_MESHES (the tables travel in 4 KiB of kernel arguments), a null table, tables that do not
 * start at 0 or descend, a mesh with nf_j outside [1, 2^24] or nv_j = 0, more than 2^28 vertices, faces or samples in all,
 * out_colors without vertex_colors, or a null required pointer (vertices, faces, out_status; out_xyz unless soff[c] == 0).  */
#define GENPC_MESH_SAMPLE_RAGGED_MAX_MESHES 128
int genpc_mesh_sample_ragged(int c, const int *voff, const int *foff, const int *soff,
                             const unsigned long long *seeds, const float *vertices,
                             const float *vertex_colors, const int *faces, float *out_xyz,
                             float *out_colors, int *out_face, float *out_bary, int *out_status,
                             void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GENPC_HIP_H */
