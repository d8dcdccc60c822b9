"""Times render_points (genpc_render_points, genpc_render_points_backward: csrc/render_grad.hip) beside the silhouette term of one
fused step of the alignment loop at the same shape, as context (no bar is attached to either).

Shapes: 1 x 16384 and 4 x 2451 points, 224 x 224, coloured clouds (a bumpy ellipsoid posed at the loop's first start), the
calling thread's blend (Pulsar's by default) and, with --blend 0, the coverage splat.  Four sides, ALTERNATING within every
repetition, each bracketed by HIP events on the stream, in one process:
  forward        render_points' forward on the posed clouds (projection, splat, image, the copy of the planes)
  backward       its backward for a dense random d L / d img (weights per pixel, gather per point, colour gradient included)
  step           genpc_pose_loss_grad_batch, mask_weight 1: one fused step (transform + projection, nearest neighbours, splat, sums,
                 gather into the 13 pose sums, finish)
  step_cd        the same with mask_weight 0: what of the step is not the silhouette term
`step - step_cd` (of the medians) is the fused loop's splat and gradient kernels at that shape.  Medians of --reps after --warmup
repetitions, with the 10th and 90th percentile, go to profiles/render_points_time.json.  Needs a GPU.

    python tools/render_points_time.py [--reps 20] [--warmup 5] [--blend 1] [--out profiles/render_points_time.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def surface(rng, n):
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (u * np.array([0.5, 0.3, 0.2])).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--blend", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_points_time.json"))
    a = ap.parse_args()
    from genpc_amd.optim_registration import diff_obj_pose as P
    P.render_tune(a.blend)
    S, radius = 224, 0.02
    result = {"size": S, "radius": radius, "blend": a.blend, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
              "shapes": {}}
    for b, n in ((1, 16384), (4, 2451)):
        rng = np.random.default_rng(100 + b)
        rest = torch.from_numpy(np.stack([surface(rng, n) for _ in range(b)])).cuda()
        part = torch.from_numpy(np.stack([surface(rng, n // 2) * np.float32(0.9) for _ in range(b)])).cuda()
        col = torch.from_numpy((0.25 + 0.75 * rng.random((b, n, 3))).astype(np.float32)).cuda()
        pcol = torch.from_numpy((0.25 + 0.75 * rng.random((b, n // 2, 3))).astype(np.float32)).cuda()
        center = rest.mean(1).contiguous()
        params = torch.tensor([[1.0, 0, 0, 0, 1, 0, 0, 0, 0, math.log(0.75)]] * b, device="cuda")
        posed = torch.stack([P.pose_transform(rest[e], center[e], params[e]) for e in range(b)])
        G = torch.from_numpy((rng.random((b, S, S, 3)) - 0.5).astype(np.float32)).cuda()
        _, planes = P.render_points_forward(posed, col, 1.1 * radius, S, a.blend)

        sides = {
            "forward": lambda: P.render_points_forward(posed, col, 1.1 * radius, S, a.blend),
            "backward": lambda: P.render_points_backward(posed, col, 1.1 * radius, S, a.blend, planes, G),
            "step": lambda: P.pose_loss_grad_batch(rest, center, params, part, radius, S, mask_weight=1.0, vert_col=col, partial_col=pcol),
            "step_cd": lambda: P.pose_loss_grad_batch(rest, center, params, part, radius, S, mask_weight=0.0, vert_col=col, partial_col=pcol),
        }
        times = {k: [] for k in sides}
        for rep in range(a.warmup + a.reps):
            for k, fn in sides.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if rep >= a.warmup:
                    times[k].append(e0.elapsed_time(e1))
        entry = {}
        for k, t in times.items():
            t = np.sort(np.array(t))
            entry[k] = {"median_ms": float(np.median(t)), "p10_ms": float(np.percentile(t, 10)), "p90_ms": float(np.percentile(t, 90))}
        entry["step_minus_step_cd_ms"] = entry["step"]["median_ms"] - entry["step_cd"]["median_ms"]
        result["shapes"]["%dx%d" % (b, n)] = entry
        print("%d x %d: " % (b, n) + "  ".join("%s %.3f (%.3f - %.3f)" % (k, v["median_ms"], v["p10_ms"], v["p90_ms"])
                                              for k, v in entry.items() if isinstance(v, dict)) + "  step - step_cd %.3f" % entry["step_minus_step_cd_ms"],
              flush=True)
    P.render_tune(-1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
