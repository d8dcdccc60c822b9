// render_ragged_plan.h -- the shape of one ragged render call (render_grad.hip genpc_render_points_ragged,
// genpc_render_points_ragged_backward), decided from the element table, the radii and the image size alone: whether the call is
// refused and why, the largest element, the grids of both directions' launches and the element counts of the scratch.  The two
// entry points branch on nothing but what render_ragged_plan returns.
// The bound on s: the element table and the radii travel BY VALUE in the arguments of the kernel that writes them to scratch
// (pose_ragged.hip's way: no copy is enqueued, nothing of the caller's host arrays is read after the entry point returns) --
// (kRenderRaggedMax + 1) ints and kRenderRaggedMax floats beside two pointers, within the 4096 bytes a kernel may take.
// Launch grids are (width for the largest element, s), or that product in one dimension where xcd_block maps the blocks; a block
// that lies wholly beyond a short element leaves.
// Host code only, no HIP: a plain C++ program can include it (tests/render_ragged_plan_check.cpp does, under the sanitizers);
// the library exports the plan as genpc_render_ragged_plan.
#pragma once
#include <stddef.h>
#include <stdio.h>

#include <algorithm>

#include "pose_plan.h"           // kQBlock, lin_grid
#include "ragged_offsets.h"

namespace genpc {

constexpr int kRenderRaggedMax = 384;                     // elements of one call
constexpr int kRenderRaggedSub = 8;                       // lanes a point of the backward gather (render_grad.hip kRenderSub)
constexpr int kRenderRaggedMaxSize = 8192;                // genpc_render_points' own
constexpr long long kRenderRaggedMaxItems = 1ll << 28;    // off[s] and s * size * size at most, as b * n and b * size * size there
static_assert((kRenderRaggedMax + 1) * sizeof(int) + kRenderRaggedMax * sizeof(float) + 2 * sizeof(void *) <= 4096,
              "the tables must fit the kernel arguments");

struct RenderRaggedAsk {
    int s = 0;                        // elements
    const int *off = nullptr;         // host, s + 1: element j owns points [off[j], off[j + 1])
    const float *radius = nullptr;    // host, s
    int size = 0, blend = 0;
    bool backward = false;
    // which of the caller's device pointers are there (forward: pts, img; backward: pts, planes, grad_img, grad_pts)
    bool pts = true, img = true, planes = true, grad_img = true, grad_pts = true;
};

struct RenderRaggedPlan {
    const char *refuse;               // null, or why the call is refused
    int refuse_element;               // the element a refusal names (its radius), or -1
    bool nothing;                     // the backward of a list without points: 1 is returned, nothing is enqueued
    int s, nmax;                      // elements; the largest element's points
    long long total;                  // off[s]
    int pixels;                       // size * size
    int g_proj;                       // forward: blocks per element of the projection, grid (g_proj, s)
    int g_pix;                        // blocks per image of render_image_kernel / render_w_kernel, grid (g_pix, s)
    int gx;                           // backward: blocks per element of the gather; the launch is gx * s blocks in one dimension
    long long grad_blocks;            // gx * s
    // element counts of the scratch
    size_t nmax_piece;                // the per-element count that sizes MaskScratch's uvr / zex: s x this >= total, at least 1
    size_t table_ints, table_floats;  // the device copies of off (s + 1) and radius (s)
    size_t w_pixels;                  // backward: W1 and W4 hold s * pixels entries each
};

inline RenderRaggedPlan render_ragged_plan(const RenderRaggedAsk &a)
{
    RenderRaggedPlan p{};
    p.refuse_element = -1;
    const auto no = [&p](const char *why) { p.refuse = why; return p; };
    if (a.s <= 0) return no("s must be positive");
    if (a.s > kRenderRaggedMax) return no("more than 384 elements in one call");
    if (!a.off) return no("off is null");
    if (!a.radius) return no("radius is null");
    if (a.size <= 0 || a.size > kRenderRaggedMaxSize) return no("size must be in 1 .. 8192");
    if (a.blend != 0 && a.blend != 1) return no("blend must be 0 or 1");
    if (const char *err = ragged_offsets_fault(a.s, a.off)) return no(err);
    for (int j = 0; j < a.s; j++)
        if (!(a.radius[j] > 0.0f)) {
            p.refuse_element = j;
            return no("the radius of every element must be positive");
        }
    if (a.off[a.s] > kRenderRaggedMaxItems || (long long)a.s * a.size * a.size > kRenderRaggedMaxItems)
        return no("off[s] and s * size * size must not exceed 2^28");
    p.s = a.s;
    p.total = a.off[a.s];
    for (int j = 0; j < a.s; j++) p.nmax = std::max(p.nmax, a.off[j + 1] - a.off[j]);
    p.pixels = a.size * a.size;
    if (a.backward) {
        if (p.total == 0) { p.nothing = true; return p; }
        if (!a.pts) return no("pts is null");
        if (!a.planes) return no("planes is null");
        if (!a.grad_img) return no("grad_img is null");
        if (!a.grad_pts) return no("grad_pts is null");
    } else {
        if (!a.img) return no("img is null");
        if (p.total > 0 && !a.pts) return no("pts is null");
    }
    p.g_proj = lin_grid(p.nmax);
    p.g_pix = lin_grid(p.pixels);
    p.gx = lin_grid((long long)p.nmax * kRenderRaggedSub);
    p.grad_blocks = (long long)p.gx * p.s;
    p.nmax_piece = (size_t)std::max(1ll, (p.total + p.s - 1) / p.s);
    p.table_ints = (size_t)p.s + 1;
    p.table_floats = (size_t)p.s;
    p.w_pixels = (size_t)p.s * (size_t)p.pixels;
    return p;
}

// "<what>" of a refused plan as the entry points record it: the radius names its element
inline void render_ragged_refusal(const RenderRaggedPlan &p, char *msg, size_t len)
{
    if (p.refuse_element >= 0)
        snprintf(msg, len, "%s (element %d)", p.refuse, p.refuse_element);
    else
        snprintf(msg, len, "%s", p.refuse ? p.refuse : "");
}

}  // namespace genpc
