"""Times the ragged alignment loop against the per-scan loop it can replace, one process, warm-up, medians:

  (a) loop      S object_pose_optimization calls, one scan after the other (runs on any commit: check out the parent, build it,
                run this file there with --only a for the parent's figure);
  (b) ragged    ONE object_pose_optimization_scans call on the same S scans;
  (d) dense     the same one call with nn_search="dense": every step's two searches by all pairs (csrc/nn_ragged_dense.hip);
  (1) S = 1     one scan through either;
  (c) reg       reg_xyz.reg_scans over S flags of a stage-2 directory (tools/reg_scans_time.py's), ragged_pose False, True with
                the grid search and True with the dense search.

The scans are reg()'s post-voxel sizes -- about 4.5 k complete against 0.9 k partial points, every scan a different size, with
colours -- and the call is reg()'s: full objective, radius 0.02, lr 0.01, iters 200, 4 starts.  Each figure is the median of
--repeats runs after --warmup, a host clock around work that ends in a read-back; where several sides are timed they alternate.
--profile runs (b) alone -- with --search dense: (d) alone --, --profile times after one warm-up, and nothing else: the run to trace.

    python tools/pose_ragged_time.py [--scans 16] [--repeats 5] [--only a|b|d|1|c] [--profile N] [--search grid|dense] [--json OUT]
"""
import argparse
import json
import math
import os
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def shape(seed, nc, np_):
    """A bumped ellipsoid surface and a one-sided, scaled, turned and moved part of it (tests/test_gpu_geometry.py's _shape)."""
    rng = np.random.default_rng(seed)
    n = max(nc, 4 * np_)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    complete = (u * np.array([0.5, 0.3, 0.2])).astype(np.float32)
    k = n // 6
    complete[:k] += np.float32([0.15, 0.1, 0.0]) * np.abs(u[:k, :1]).astype(np.float32)
    th = math.radians(12.0)
    Rt = np.array([[math.cos(th), 0, math.sin(th)], [0, 1, 0], [-math.sin(th), 0, math.cos(th)]])
    c = complete.mean(0)
    full = ((complete - c) * 0.9) @ Rt.T + c + np.array([0.02, -0.01, 0.015])
    partial = full[full[:, 2] > -0.05][:np_].astype(np.float32)
    assert len(partial) == np_
    return complete[:nc].copy(), partial, rng.random((nc, 3)).astype(np.float32), rng.random((np_, 3)).astype(np.float32)


def alternate(fns, warmup, repeats):
    """(median, min, max) in ms for several callables, one run of each in turn (each ends in its own read-back)."""
    for _ in range(warmup):
        for f in fns:
            f()
    ts = [[] for _ in fns]
    for _ in range(repeats):
        for k, f in enumerate(fns):
            t0 = time.perf_counter()
            f()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    out = []
    for t in ts:
        t.sort()
        out.append((t[len(t) // 2], t[0], t[-1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default="abd1c")
    ap.add_argument("--search", default="grid", choices=("grid", "dense"))
    ap.add_argument("--profile", type=int, default=0)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    from genpc_amd.optim_registration import diff_obj_pose as POSE
    if not torch.cuda.is_available():
        raise SystemExit("pose_ragged_time: needs a GPU (a CPU run times nothing of interest)")
    s = args.scans
    sizes = [(4493 + 37 * (j % 7) - 53 * (j % 5), 886 + 11 * (j % 6) - 17 * (j % 4)) for j in range(s)]
    raw = [shape(40 + j, *sizes[j]) for j in range(s)]
    C, P, CC, PC = ([torch.from_numpy(r[k]).cuda() for r in raw] for k in range(4))
    kw = dict(radius=0.02, lr=0.01, iters=200, render_size=224)
    res = {"scans": s, "sizes": sizes, "device": torch.cuda.get_device_name(0), "call": dict(kw, starts=4)}
    has_ragged = hasattr(POSE, "object_pose_optimization_scans")
    import inspect
    has_dense = has_ragged and "nn_search" in inspect.signature(POSE.object_pose_optimization_scans).parameters

    def loop():
        return [POSE.object_pose_optimization(C[j], P[j], complete_col=CC[j], partial_col=PC[j], **kw) for j in range(s)]

    def ragged():
        return POSE.object_pose_optimization_scans(C, P, complete_cols=CC, partial_cols=PC, **kw)

    def dense():
        return POSE.object_pose_optimization_scans(C, P, complete_cols=CC, partial_cols=PC, nn_search="dense", **kw)

    if args.profile:
        traced = dense if args.search == "dense" else ragged
        traced()
        for _ in range(args.profile):
            traced()
        return
    if has_ragged:
        import ctypes
        from genpc_amd import _lib
        off = lambda k: (ctypes.c_int * (s + 1))(*([0] + list(np.cumsum([z[k] for z in sizes]))))      # noqa: E731
        out = (ctypes.c_int * 16)()
        _lib.lib.genpc_pose_ragged_plan(s, ctypes.cast(off(0), ctypes.c_void_p), ctypes.cast(off(1), ctypes.c_void_p), 4, 1, 224, 0.02, 256,
                                        ctypes.cast(out, ctypes.c_void_p))
        res["plan"] = list(out)
        # transform | search, build, search | splat, sums, [weights], gradient (pose_grad rides or is a launch of its own) | update
        res["launches_per_step"] = 3 + 3 + (0 if out[8] else 1) + (0 if out[7] else 1) + 1 + 1
        if has_dense:
            res["launches_per_step_dense"] = res["launches_per_step"] - 1          # two searches and no build
    sides = [(k, n, f) for k, n, f, ok in (("a", "loop_ms", loop, True), ("b", "ragged_ms", ragged, has_ragged), ("d", "ragged_dense_ms", dense, has_dense))
             if k in args.only and ok]
    if sides:          # the sides that are asked for alternate in one process
        for (_, name, _), t in zip(sides, alternate([f for _, _, f in sides], args.warmup, args.repeats)):
            res[name] = t
    if "1" in args.only:
        one = [lambda: POSE.object_pose_optimization(C[0], P[0], complete_col=CC[0], partial_col=PC[0], **kw)]
        if has_ragged:
            one.append(lambda: POSE.object_pose_optimization_scans(C[:1], P[:1], complete_cols=CC[:1], partial_cols=PC[:1], **kw))
        if has_dense:
            one.append(lambda: POSE.object_pose_optimization_scans(C[:1], P[:1], complete_cols=CC[:1], partial_cols=PC[:1], nn_search="dense", **kw))
        t = alternate(one, args.warmup, args.repeats)
        res["single_1_ms"] = t[0]
        if has_ragged:
            res["ragged_1_ms"] = t[1]
        if has_dense:
            res["ragged_dense_1_ms"] = t[2]
    if "c" in args.only and has_ragged:
        from conftest import write_glb
        from reg_scans_time import ellipsoid
        from genpc_amd import reg_xyz as R
        from genpc_amd.utils import dataUtils as D, mesh_io as M
        root = args.dir or tempfile.mkdtemp(prefix="pose_ragged_time_")
        cfg = SimpleNamespace(output_path=root, device="cuda", generative_model="trellis", dataset="redwood")
        flags = ["%05d" % (100 + j) for j in range(s)]
        for j, flag in enumerate(flags):          # (tools/reg_scans_time.py's directory)
            base = os.path.join(root, flag)
            os.makedirs(base, exist_ok=True)
            verts, faces, cols = ellipsoid(200 - 4 * j, 120 + 2 * j)
            glb = os.path.join(base, flag + "_trellis.glb")
            write_glb(glb, verts, faces, cols, indices_u16=False)
            pts_j, pc = M.glb2point_gpu(glb, num_points=12000 + 500 * j, seed=5 + j)
            pts_j, pc = pts_j.cpu().numpy(), pc.cpu().numpy()
            front = pts_j[:, 2] > -0.02
            partial = (pts_j[front] * 0.88 + np.array([0.015, -0.01, 0.01])).astype(np.float32)
            D.save_ply_xyzrgb(partial, pc[front], os.path.join(base, "color_point.ply"))
        cwd = os.getcwd()
        os.chdir(root)
        try:
            fns = [lambda: R.reg_scans(cfg, flags, seed=7), lambda: R.reg_scans(cfg, flags, seed=7, ragged_pose=True)]
            if has_dense:
                fns.append(lambda: R.reg_scans(cfg, flags, seed=7, ragged_pose=True, nn_search="dense"))
            t = alternate(fns, 1, args.repeats)
            res["reg_scans_per_scan_pose_ms"], res["reg_scans_ragged_pose_ms"] = t[0], t[1]
            if has_dense:
                res["reg_scans_ragged_dense_pose_ms"] = t[2]
        finally:
            os.chdir(cwd)
    for k in sorted(res):
        if k.endswith("_ms"):
            print("%-28s median %10.3f ms   (min %.3f, max %.3f)" % ((k[:-3],) + tuple(res[k])))
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
