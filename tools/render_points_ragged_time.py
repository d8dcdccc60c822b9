"""Times render_points_ragged (genpc_render_points_ragged, genpc_render_points_ragged_backward: csrc/render_grad.hip) beside what the
equal-size entry points offer for the same job: one call per cloud.  As context -- no bar is attached, no default depends on it.

Shape: 16 coloured clouds of 2000 to 3000 points (bumpy ellipsoids), 224 x 224, a radius per cloud, both blends, forward and
backward for a dense random d L / d img.  Two sides, ALTERNATING within every repetition, each bracketed by HIP events on the
stream, in one process:
  ragged   one genpc_render_points_ragged call / one genpc_render_points_ragged_backward call for the 16 clouds
  loop     16 genpc_render_points / genpc_render_points_backward calls with b = 1, one after the other
Both sides go through the Python wrappers of genpc_amd.optim_registration.diff_obj_pose (output allocation included, the same on
both sides per image).  Medians of --reps after --warmup repetitions, with the 10th and 90th percentile, go to
profiles/render_points_ragged_time.json.  Needs a GPU.

    python tools/render_points_ragged_time.py [--reps 20] [--warmup 5] [--out profiles/render_points_ragged_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def surface(rng, n):
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (u * np.array([0.5, 0.3, 0.2]) * (0.6 + 0.4 * rng.random())).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_points_ragged_time.json"))
    a = ap.parse_args()
    from genpc_amd.optim_registration import diff_obj_pose as P
    S, s = 224, 16
    rng = np.random.default_rng(2024)
    sizes = [int(v) for v in rng.integers(2000, 3001, s)]
    radii = [0.018 + 0.0005 * j for j in range(s)]
    clouds = [torch.from_numpy(surface(rng, n)).cuda() for n in sizes]
    cols = [torch.from_numpy((0.25 + 0.75 * rng.random((n, 3))).astype(np.float32)).cuda() for n in sizes]
    off = [0]
    for n in sizes:
        off.append(off[-1] + n)
    pts, col = torch.cat(clouds).contiguous(), torch.cat(cols).contiguous()
    one_p, one_c = [c[None].contiguous() for c in clouds], [c[None].contiguous() for c in cols]
    G = torch.from_numpy((rng.random((s, S, S, 3)) - 0.5).astype(np.float32)).cuda()
    one_G = [G[j:j + 1].contiguous() for j in range(s)]
    result = {"size": S, "clouds": s, "sizes": sizes, "radii": radii, "reps": a.reps, "warmup": a.warmup,
              "device": torch.cuda.get_device_name(0), "blends": {}}
    for blend in (1, 0):
        _, planes = P.render_points_ragged_forward(pts, off, col, radii, S, blend)
        one_pl = [P.render_points_forward(one_p[j], one_c[j], radii[j], S, blend)[1] for j in range(s)]
        assert all(torch.equal(one_pl[j][0], planes[j]) for j in range(s))          # the two sides draw the same images

        def loop_forward():
            for j in range(s):
                P.render_points_forward(one_p[j], one_c[j], radii[j], S, blend)

        def loop_backward():
            for j in range(s):
                P.render_points_backward(one_p[j], one_c[j], radii[j], S, blend, one_pl[j], one_G[j])
        sides = {
            "forward_ragged": lambda: P.render_points_ragged_forward(pts, off, col, radii, S, blend),
            "forward_loop": loop_forward,
            "backward_ragged": lambda: P.render_points_ragged_backward(pts, off, col, radii, S, blend, planes, G),
            "backward_loop": loop_backward,
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
        entry["forward_loop_over_ragged"] = entry["forward_loop"]["median_ms"] / entry["forward_ragged"]["median_ms"]
        entry["backward_loop_over_ragged"] = entry["backward_loop"]["median_ms"] / entry["backward_ragged"]["median_ms"]
        result["blends"][str(blend)] = entry
        print("blend %d: " % blend + "  ".join("%s %.3f (%.3f - %.3f)" % (k, v["median_ms"], v["p10_ms"], v["p90_ms"])
                                              for k, v in entry.items() if isinstance(v, dict)) +
              "  loop / ragged: forward %.2f backward %.2f" % (entry["forward_loop_over_ragged"], entry["backward_loop_over_ragged"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
