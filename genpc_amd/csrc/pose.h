// pose.h -- the device code the alignment loop's translation units share (pose.hip, mask_render.hip, mask_loss.hip): the 7-DoF pose
// model, the Adam step of one element, the hand-over words of the loop's two streams, and the Chamfer gradient's body, which
// mask_grad_kernel (mask_loss.hip) carries along.  Every file is compiled by itself without relocatable device code, so what is
// shared is __forceinline__ and lives here, once.
#pragma once
#include "common.h"
#include "pose_plan.h"      // kQBlock, lin_grid
#include "ragged_table.h"   // RaggedTable: a ragged call's tables by value (pose_ragged.hip)

#include <math.h>

namespace genpc {

// doubles per scan: [0..12] gradient sums, [13,14] Chamfer sums, [15] mask loss, [16..18] sum I_ch, [19..21] sum I_ch^2,
// [22..25] mse / bce / intersection / sum m, [26 + 6 ch + k] the six gradient sums of channel ch (mask_sums_kernel)
constexpr int kAcc = 48;

// pytorch3d.transforms.rotation_6d_to_matrix (rows b1, b2, b1 x b2); F.normalize eps 1e-12
__device__ __forceinline__ void rot6d_to_matrix(const float *d6, float *R)
{
    const float a1x = d6[0], a1y = d6[1], a1z = d6[2], a2x = d6[3], a2y = d6[4], a2z = d6[5];
    float n1 = sqrtf(a1x * a1x + a1y * a1y + a1z * a1z);
    n1 = n1 > 1e-12f ? n1 : 1e-12f;
    const float b1x = a1x / n1, b1y = a1y / n1, b1z = a1z / n1;
    const float dt = b1x * a2x + b1y * a2y + b1z * a2z;
    float b2x = a2x - dt * b1x, b2y = a2y - dt * b1y, b2z = a2z - dt * b1z;
    float n2 = sqrtf(b2x * b2x + b2y * b2y + b2z * b2z);
    n2 = n2 > 1e-12f ? n2 : 1e-12f;
    b2x /= n2; b2y /= n2; b2z /= n2;
    R[0] = b1x; R[1] = b1y; R[2] = b1z;
    R[3] = b2x; R[4] = b2y; R[5] = b2z;
    R[6] = b1y * b2z - b1z * b2y;
    R[7] = b1z * b2x - b1x * b2z;
    R[8] = b1x * b2y - b1y * b2x;
}

__device__ __forceinline__ void pose_point(const float *R, float s, const float *c, const float *t, float vx, float vy,
                                           float vz, float *o)
{
    const float lx = __fmul_rn(vx - c[0], s), ly = __fmul_rn(vy - c[1], s), lz = __fmul_rn(vz - c[2], s);
    o[0] = __fadd_rn(__fadd_rn(__fmaf_rn(R[2], lz, __fmaf_rn(R[1], ly, __fmul_rn(R[0], lx))), c[0]), t[0]);
    o[1] = __fadd_rn(__fadd_rn(__fmaf_rn(R[5], lz, __fmaf_rn(R[4], ly, __fmul_rn(R[3], lx))), c[1]), t[1]);
    o[2] = __fadd_rn(__fadd_rn(__fmaf_rn(R[8], lz, __fmaf_rn(R[7], ly, __fmul_rn(R[6], lx))), c[2]), t[2]);
}

// Waiting for a count another stream's kernel publishes (bounded: ~2 s; a wait that gives up marks ctr[2] and the results of the call
// become NaN).  Acquire: what the counted blocks wrote before their increment is visible afterwards.
__device__ __forceinline__ bool pose_wait_count(unsigned *ctr, int which, unsigned target)
{
    for (long long spin = 0; spin < (1ll << 24); spin++) {
        if ((int)(__hip_atomic_load(ctr + which, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) >= 0) {
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
            return true;
        }
        __builtin_amdgcn_s_sleep(8);
    }
    __hip_atomic_store(ctr + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return false;
}
// every block of a counted launch, after its work: what it wrote is visible to whoever sees the count
__device__ __forceinline__ void pose_publish_block(unsigned *ctr, int which)
{
    __syncthreads();
    if (threadIdx.x == 0) {
        __atomic_thread_fence(__ATOMIC_RELEASE);
        __hip_atomic_fetch_add(ctr + which, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Where element e's points lie in an array packed element by element -- THE one statement of it for every per-point kernel of the
// loop.  Without a table: n points at e * n, the equal-size calls' arithmetic.  With one (a ragged call; elements + 1 ints on the
// device, csrc/pose_ragged.hip): off[e + 1] - off[e] points at off[e].  e is uniform over the block, so the two reads are scalar
// loads, and a count taken from here is block-uniform: it may bound a loop with barriers in it.
struct PoseSpan {
    size_t base;
    int n;
};
__device__ __forceinline__ PoseSpan pose_span(const int *__restrict__ off, int e, int n)
{
    if (!off) return PoseSpan{(size_t)e * n, n};
    const int o = off[e];
    return PoseSpan{(size_t)o, off[e + 1] - o};
}

// accum[0..8] = dL/dR (row-major), [9] = dL/ds, [10..12] = dL/dt, [13] = sum sqrt(d1),
// [14] = sum sqrt(d2).  Thread t < nc: term of complete point t (pts -> partial);
// nc <= t < nc+np: term of partial point t-nc (partial -> pts), attributed to the
// complete point it matched.
struct PoseGradArgs {          // pose_grad_kernel's arguments, for the launch that carries it along (mask_grad_kernel)
    int nc, cstride, pstride, np;
    const float *v, *center, *params, *partial, *d1, *d2;
    const int *i1, *i2;
    float cd_weight;
    double *accum;
    int gx;                    // blocks per batch element; 0: nothing rides along
    const int *coff, *poff;    // a ragged call's element tables (pose_span), or null
};
__device__ __forceinline__ void pose_grad_body(int bx, int gdx, int e, int nc, const float *__restrict__ v,
                                               const float *__restrict__ center, int cstride,
                                               const float *__restrict__ params, int pstride, int np,
                                               const float *__restrict__ partial,
                                               const float *__restrict__ d1, const int *__restrict__ i1,
                                               const float *__restrict__ d2, const int *__restrict__ i2,
                                               float cd_weight, double *__restrict__ accum, double (*red)[kQBlock / kWave],
                                               const int *__restrict__ coff = nullptr, const int *__restrict__ poff = nullptr)
{
    const PoseSpan sc = pose_span(coff, e, nc), sq = pose_span(poff, e, np);
    nc = sc.n; np = sq.n;                                    // (the weights 1 / nc, 0.5 / np below are the element's own)
    if (coff && bx * kQBlock >= nc + np) return;             // a short element of a ragged call: the whole block leaves
    v += sc.base * 3;
    partial += sq.base * 3;
    d1 += sc.base; i1 += sc.base;
    d2 += sq.base; i2 += sq.base;
    center += (size_t)e * cstride;
    params += (size_t)e * pstride;
    accum += (size_t)e * kAcc;
    float R[9];
    rot6d_to_matrix(params, R);
    const float s = expf(params[9]);
    const float c[3] = {center[0], center[1], center[2]};
    const float t[3] = {params[6], params[7], params[8]};
    double a[15];
#pragma unroll
    for (int k = 0; k < 15; k++) a[k] = 0.0;
    for (int e = bx * kQBlock + threadIdx.x; e < nc + np; e += gdx * kQBlock) {
        int j, k;
        float d;
        double w;
        if (e < nc) {
            j = e; k = i1[e]; d = d1[e];
            a[13] += (double)sqrtf(d);
            w = (double)cd_weight / nc;
        } else {
            k = e - nc; j = i2[k]; d = d2[k];
            a[14] += (double)sqrtf(d);
            w = (double)cd_weight * 0.5 / np;
        }
        if (d == 0.0f || (j | k) < 0) continue;     // torch: 0.5/sqrt(0) * 0 = NaN; no gradient here  (index -1: the ragged search's answer to a non-finite query, its distance NaN)
        w *= 1.0 / sqrt((double)d);  // d sqrt(d)/dd * 2 (from d |p-q|^2 / dp)
        const float vx = v[(size_t)j * 3 + 0], vy = v[(size_t)j * 3 + 1], vz = v[(size_t)j * 3 + 2];
        float p[3];
        pose_point(R, s, c, t, vx, vy, vz, p);
        const double g[3] = {w * (double)(p[0] - partial[(size_t)k * 3 + 0]),
                             w * (double)(p[1] - partial[(size_t)k * 3 + 1]),
                             w * (double)(p[2] - partial[(size_t)k * 3 + 2])};
        const double l[3] = {(double)(vx - c[0]), (double)(vy - c[1]), (double)(vz - c[2])};
#pragma unroll
        for (int r = 0; r < 3; r++) {
            a[10 + r] += g[r];
#pragma unroll
            for (int q = 0; q < 3; q++) a[r * 3 + q] += g[r] * (double)s * l[q];
            a[9] += g[r] * ((double)R[r * 3 + 0] * l[0] + (double)R[r * 3 + 1] * l[1] + (double)R[r * 3 + 2] * l[2]);
        }
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 15; k++) {
        const double x = wave_sum63(a[k]);
        if (lane == kWave - 1) red[k][wave] = x;
    }
    __syncthreads();
    if (threadIdx.x < 15) {
        double x = 0.0;
#pragma unroll
        for (int w2 = 0; w2 < kQBlock / kWave; w2++) x += red[threadIdx.x][w2];
        atomicAdd(&accum[threadIdx.x], x);
    }
}

struct PoseState {       // device-resident
    float params[10];
    float m[10];
    float v[10];
    float grad[10];
    float loss[4];       // total, cd, ortho_err, mask_loss
    float local_best;
    float best_loss;
    float best_params[10];
    int step;            // Adam step of the current start (1-based after the first update)
    int patience_counter;   // steps since local_best last improved (diff_obj_pose.py:549-556)
    int stopped;         // the start has run out of patience: its parameters are frozen for the rest of its iterations
};
constexpr int kPosePatience = 300;      // diff_obj_pose.py:530

// One thread, one batch element: finish the gradient (orthogonality term + 6D backward), optionally take the Adam step,
// record the loss; `clear`: zero the element's accumulators.  S may be a private copy of the state (the fused form below).
__device__ __forceinline__ void pose_update_one(PoseState *S, double *accum, int nc, int np, float cd_weight, float reg_weight, float lr,
                                                int do_step, float *history_slot, bool clear)
{
    float Rf[9];
    rot6d_to_matrix(S->params, Rf);
    const double s = (double)expf(S->params[9]);
    double gR[9];
    for (int k = 0; k < 9; k++) gR[k] = accum[k];
    const double cd = accum[13] / nc + 0.5 * accum[14] / np;
    double E[9], err2 = 0.0;
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            double e = 0.0;
            for (int k = 0; k < 3; k++) e += (double)Rf[a * 3 + k] * (double)Rf[b * 3 + k];
            e -= (a == b) ? 1.0 : 0.0;
            E[a * 3 + b] = e;
            err2 += e * e;
        }
    const double err = sqrt(err2);
    if (err > 0.0)
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) {
                double acc = 0.0;
                for (int k = 0; k < 3; k++) acc += E[a * 3 + k] * (double)Rf[k * 3 + b];
                gR[a * 3 + b] += (double)reg_weight * 2.0 * acc / err;
            }
    // Gram-Schmidt backward (double)
    const float *d6 = S->params;
    const double a1[3] = {d6[0], d6[1], d6[2]}, a2[3] = {d6[3], d6[4], d6[5]};
    const double n1 = sqrt(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]);
    const double b1[3] = {a1[0] / n1, a1[1] / n1, a1[2] / n1};
    const double dt = b1[0] * a2[0] + b1[1] * a2[1] + b1[2] * a2[2];
    const double u[3] = {a2[0] - dt * b1[0], a2[1] - dt * b1[1], a2[2] - dt * b1[2]};
    const double n2 = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    const double b2[3] = {u[0] / n2, u[1] / n2, u[2] / n2};
    const double *g1 = gR, *g2 = gR + 3, *g3 = gR + 6;
    double gb1[3], gb2[3];
    gb1[0] = g1[0] + (b2[1] * g3[2] - b2[2] * g3[1]);
    gb1[1] = g1[1] + (b2[2] * g3[0] - b2[0] * g3[2]);
    gb1[2] = g1[2] + (b2[0] * g3[1] - b2[1] * g3[0]);
    gb2[0] = g2[0] + (g3[1] * b1[2] - g3[2] * b1[1]);
    gb2[1] = g2[1] + (g3[2] * b1[0] - g3[0] * b1[2]);
    gb2[2] = g2[2] + (g3[0] * b1[1] - g3[1] * b1[0]);
    const double dot2 = gb2[0] * b2[0] + gb2[1] * b2[1] + gb2[2] * b2[2];
    const double gu[3] = {(gb2[0] - dot2 * b2[0]) / n2, (gb2[1] - dot2 * b2[1]) / n2, (gb2[2] - dot2 * b2[2]) / n2};
    const double gub1 = gu[0] * b1[0] + gu[1] * b1[1] + gu[2] * b1[2];
    const double ga2[3] = {gu[0] - gub1 * b1[0], gu[1] - gub1 * b1[1], gu[2] - gub1 * b1[2]};
    for (int k = 0; k < 3; k++) gb1[k] += -dt * gu[k] - gub1 * a2[k];
    const double dot1 = gb1[0] * b1[0] + gb1[1] * b1[1] + gb1[2] * b1[2];
    float grad[10];
    for (int k = 0; k < 3; k++) grad[k] = (float)((gb1[k] - dot1 * b1[k]) / n1);
    for (int k = 0; k < 3; k++) grad[3 + k] = (float)ga2[k];
    for (int k = 0; k < 3; k++) grad[6 + k] = (float)accum[10 + k];
    grad[9] = (float)(accum[9] * s);
    // accum[15]: mask_weight * mask_loss of this step (mask_loss_kernel), 0 without the mask term
    const float loss = (float)((double)cd_weight * cd + (double)reg_weight * err + accum[15]);
    for (int k = 0; k < 10; k++) S->grad[k] = grad[k];
    S->loss[0] = loss;
    S->loss[1] = (float)cd;
    S->loss[2] = (float)err;
    S->loss[3] = (float)accum[15];
    if (clear)
        for (int k = 0; k < kAcc; k++) accum[k] = 0.0;
    // Early stop (diff_obj_pose.py:529-556): the reference leaves a start's loop once `patience` steps in a row failed to
    // improve its best loss.  The launches of a start are enqueued up front here, so a stopped start keeps its parameters
    // and its best loss through the remaining launches (history: NaN = "iteration not run").
    if (do_step && S->stopped) {
        if (history_slot) *history_slot = __builtin_nanf("");
        return;
    }
    if (history_slot) *history_slot = loss;
    if (!do_step) return;
    if (loss < S->local_best) {       // :549-553 (the optimizer step below has been taken by then, as here)
        S->local_best = loss;
        S->patience_counter = 0;
    } else if (++S->patience_counter > kPosePatience) {
        S->stopped = 1;               // :554-556: break AFTER this iteration's step
    }
    // torch.optim.Adam, three groups: lr, 0.2 lr, 0.1 lr (diff_obj_pose.py:524-528)
    const int step = ++S->step;
    const double be1 = 0.9, be2 = 0.999, eps = 1e-8;
    const double bc1 = 1.0 - pow(be1, (double)step), bc2 = 1.0 - pow(be2, (double)step);
    for (int k = 0; k < 10; k++) {
        const double l = k < 6 ? (double)lr : (k < 9 ? (double)lr * 0.2 : (double)lr * 0.1);
        S->m[k] = (float)(be1 * S->m[k] + (1.0 - be1) * grad[k]);
        S->v[k] = (float)(be2 * S->v[k] + (1.0 - be2) * (double)grad[k] * grad[k]);
        const double denom = sqrt((double)S->v[k]) / sqrt(bc2) + eps;
        S->params[k] = (float)(S->params[k] - (l / bc1) * (S->m[k] / denom));
    }
}

// The update of step k fused into the transform of step k + 1 (round 6: one launch and one kernel boundary less per Adam step).
// Every block of the transform recomputes the update of ITS batch element from the previous state and the previous step's
// accumulators (thread 0; the same arithmetic on the same inputs: every block gets the same parameters), block 0 of the element
// writes the new state to the OTHER state buffer (the other blocks are still reading the old one), records the loss and zeroes
// the accumulators the new step is about to use (their last reader was the previous transform).
struct PoseFuse {
    const PoseState *S_in;
    PoseState *S_out;
    double *acc_in, *acc_zero;
    int do_update, nc, np;
    float lr;
    float *history;          // slot of the step being finished (element 0), or null
    int hstride;
    // the hand-over between the loop's two streams through device words instead of events (below): ctr[0] counts finished blocks of
    // the transforms, ctr[1] of pose_grad, ctr[2] != 0: a wait gave up
    unsigned *ctr;
    unsigned pg_target;      // the update waits for ctr[1] to reach this (the Chamfer half's sums are complete)
};

__device__ __forceinline__ const float *pose_fused_params(const PoseFuse &fu, int e, const float *params, float *s_par)
{
    if (!fu.do_update) return params;
    if (threadIdx.x == 0) {
        bool gave_up = false;
        if (fu.ctr) gave_up = !pose_wait_count(fu.ctr, 1, fu.pg_target) || __hip_atomic_load(fu.ctr + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
        PoseState st = fu.S_in[e];
        const bool lead = blockIdx.x == 0;
        pose_update_one(&st, fu.acc_in + (size_t)e * kAcc, fu.nc, fu.np, 3.0f, 0.001f, fu.lr, 1,
                        lead && fu.history ? fu.history + (size_t)e * fu.hstride : (float *)nullptr, false);
        if (gave_up)
            for (int k = 0; k < 10; k++) st.params[k] = __builtin_nanf("");          // (a hand-over that timed out: visibly)
#pragma unroll
        for (int k = 0; k < 10; k++) s_par[k] = st.params[k];
        if (lead) {
            fu.S_out[e] = st;
            for (int k = 0; k < kAcc; k++) fu.acc_zero[(size_t)e * kAcc + k] = 0.0;
        }
    }
    __syncthreads();
    return s_par;
}

// pose_ragged.hip -- the two launches of a ragged call that are not the loop's own (host functions: every file is compiled by itself).
// The element tables (qoff: complete clouds, toff: partial clouds; c + 1 entries each) written to coff_e / poff_e on the device;
// the scans' clouds and colours (src / dst: complete, partial, complete colours, partial colours; null = absent) copied once
// per start, packed by the element tables.  width: blocks per scan.
int pose_ragged_tables(const RaggedTable &elements, int *coff_e, int *poff_e, hipStream_t st);
int pose_ragged_replicate(const RaggedTable &scans, int starts, int width, const float *const src[4], float *const dst[4], hipStream_t st);

}  // namespace genpc
