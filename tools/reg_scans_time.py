"""Times the two multi-scan entry points against the loops they replace, both sides in the same process, alternating:

  (a) sample    mesh_io.sample_surfaces_gpu for S meshes of about 2 * 10^5 faces x 163 840 samples with colours (arrays
                resident on the device) against the loop of sample_surface_gpu; and the library calls alone between device
                events, on preallocated buffers: one genpc_mesh_sample_ragged against S genpc_mesh_sample.
  (b) reg       reg_xyz.reg_scans over S flags of a stage-2 directory against the loop of reg, seed 7, with the pose
                initialisation (diff_init=True) and without it: the difference is the pose initialisation's share, the one
                stage that stays per scan.  The directory is written under --dir from seeded meshes (bumped ellipsoids of
                different resolutions) and their front halves as partial clouds.  S = 1 is timed too.

Each figure is the median of --repeats runs after --warmup, a host clock around work that ends in a device synchronise
(device events for the library calls).  Nothing is asserted but that the two sides return the same bits where they must.

    python tools/reg_scans_time.py [--scans 16] [--repeats 5] [--dir DIR] [--json OUT]
"""
import argparse
import json
import os
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def ellipsoid(nu, nv, radii=(0.45, 0.3, 0.2)):
    """A bumped ellipsoid of 2 nu (nv - 1) triangles with vertex colours (tests/test_gpu_mesh_sample.py's, without its loop)."""
    u = np.linspace(0, 2 * np.pi, nu, endpoint=False)
    v = np.linspace(0.05, np.pi - 0.05, nv)
    uu, vv = np.meshgrid(u, v)
    verts = np.stack([radii[0] * np.cos(uu) * np.sin(vv), radii[1] * np.cos(vv), radii[2] * np.sin(uu) * np.sin(vv)], -1).reshape(-1, 3)
    verts[:, 0] += 0.12 * (verts[:, 1] > 0.1)
    j, i = np.meshgrid(np.arange(nv - 1), np.arange(nu), indexing="ij")
    a, b = (j * nu + i).reshape(-1), (j * nu + (i + 1) % nu).reshape(-1)
    faces = np.stack([np.stack([a, b, a + nu], -1), np.stack([b, b + nu, a + nu], -1)], 1).reshape(-1, 3)
    cols = 0.2 + 0.8 * (verts - verts.min(0)) / (verts.max(0) - verts.min(0))
    return verts.astype(np.float32), faces.astype(np.int32), cols.astype(np.float32)


def alternate(fns, warmup, repeats, sync):
    """(median, min, max) in ms for several callables, one run of each in turn, so that drift of the machine falls on all of them alike."""
    for _ in range(warmup):
        for f in fns:
            f()
    sync()
    ts = [[] for _ in fns]
    for _ in range(repeats):
        for k, f in enumerate(fns):
            t0 = time.perf_counter()
            f()
            sync()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    out = []
    for t in ts:
        t.sort()
        out.append((t[len(t) // 2], t[0], t[-1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=16)
    ap.add_argument("--samples", type=int, default=163840)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop", type=int, default=20, help="library calls (ragged) / rounds of S calls (loop) between two device events")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    from conftest import write_glb
    from genpc_amd import _lib, reg_xyz as R
    from genpc_amd.utils import dataUtils as D, mesh_io as M
    if not torch.cuda.is_available():
        raise SystemExit("reg_scans_time: needs a GPU (a CPU run times nothing of interest)")
    dev = torch.device("cuda", torch.cuda.current_device())
    sync = torch.cuda.synchronize
    s, n = args.scans, args.samples
    res = {"scans": s, "samples": n, "device": torch.cuda.get_device_name(dev)}

    # (a) the sampling: S meshes of about 2 * 10^5 faces each, every one a different size
    meshes = [ellipsoid(400 - 3 * j, 250 + j) for j in range(s)]
    res["faces"] = [int(len(m[1])) for m in meshes]
    on_dev = [tuple(torch.from_numpy(a).to(dev) for a in m) for m in meshes]
    seeds = [100 + j for j in range(s)]

    def ragged():
        return M.sample_surfaces_gpu(on_dev, n, seeds)

    def loop():
        return [M.sample_surface_gpu(V, F, n, seeds[j], colors=C) for j, (V, F, C) in enumerate(on_dev)]
    a, b = ragged(), loop()
    assert all(torch.equal(x, y) for ta, tb in zip(a, b) for x, y in zip(ta, tb))
    res["sample_ragged_ms"], res["sample_loop_ms"] = alternate([ragged, loop], args.warmup, args.repeats, sync)
    res["sample_ragged_1_ms"], res["sample_loop_1_ms"] = alternate(
        [lambda: M.sample_surfaces_gpu(on_dev[:1], n, seeds[:1]), lambda: M.sample_surface_gpu(*on_dev[0][:2], n, seeds[0], colors=on_dev[0][2])],
        args.warmup, args.repeats, sync)
    # the library calls alone, preallocated, between device events
    import ctypes
    L, p = _lib.lib, _lib.ptr
    V, F, C = [torch.cat([m[k] for m in on_dev]).contiguous() for k in range(3)]
    voff, foff = [0], [0]
    for m in on_dev:
        voff.append(voff[-1] + len(m[0]))
        foff.append(foff[-1] + len(m[1]))
    soff = [n * j for j in range(s + 1)]
    tabs = [(ctypes.c_int * (s + 1))(*o) for o in (voff, foff, soff)]
    sd = (ctypes.c_ulonglong * s)(*seeds)
    pts, col = torch.empty(n * s, 3, device=dev), torch.empty(n * s, 3, device=dev)
    fi, st = torch.empty(n * s, dtype=torch.int32, device=dev), torch.empty(s, dtype=torch.int32, device=dev)
    ws = [torch.empty(L.genpc_mesh_sample_bytes(len(m[1])), dtype=torch.uint8, device=dev) for m in on_dev]
    cast = lambda t: ctypes.cast(t, ctypes.c_void_p)

    def call_ragged():
        return _lib.on_device_of(V, L.genpc_mesh_sample_ragged, s, cast(tabs[0]), cast(tabs[1]), cast(tabs[2]), cast(sd), p(V), p(C), p(F),
                                 p(pts), p(col), p(fi), p(None), p(st))

    def call_loop():
        for j, (v, f, c) in enumerate(on_dev):
            sl = slice(n * j, n * (j + 1))
            _lib.on_device_of(v, L.genpc_mesh_sample, len(v), p(v), p(c), len(f), p(f), n, seeds[j], p(pts[sl]), p(col[sl]), p(fi[sl]),
                              p(None), p(st[j:j + 1]), p(ws[j]))
        return 1
    for name, fn in (("kernels_ragged_us", call_ragged), ("kernels_loop_us", call_loop)):
        for _ in range(3):
            assert fn() == 1
        sync()
        per = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.loop):
                fn()
            e1.record()
            e1.synchronize()
            per.append(e0.elapsed_time(e1) / args.loop * 1e3)
        per.sort()
        res[name] = (per[len(per) // 2], per[0], per[-1])
        assert st.tolist() == [1] * s

    # (b) reg over S flags
    root = args.dir or tempfile.mkdtemp(prefix="reg_scans_time_")
    cfg = SimpleNamespace(output_path=root, device="cuda", generative_model="trellis", dataset="redwood")
    flags = ["%05d" % (100 + j) for j in range(s)]
    for j, flag in enumerate(flags):
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
    os.chdir(root)                       # reg's pose initialisation writes its side-effect files into the working directory
    try:
        for pose in (True, False):
            key = "pose" if pose else "nopose"
            fns = [lambda: R.reg_scans(cfg, flags, seed=7, diff_init=pose), lambda: [R.reg(cfg, f, seed=7, diff_init=pose) for f in flags]]
            res["reg_scans_%s_ms" % key], res["reg_loop_%s_ms" % key] = alternate(fns, 1, args.repeats, sync)
            one = [lambda: R.reg_scans(cfg, flags[:1], seed=7, diff_init=pose), lambda: R.reg(cfg, flags[0], seed=7, diff_init=pose)]
            res["reg_scans_1_%s_ms" % key], res["reg_loop_1_%s_ms" % key] = alternate(one, 1, args.repeats, sync)
    finally:
        os.chdir(cwd)
    for k in sorted(res):
        if k.endswith("_ms"):
            print("%-24s median %10.3f ms   (min %.3f, max %.3f)" % ((k[:-3],) + tuple(res[k])))
        elif k.endswith("_us"):
            print("%-24s median %10.1f us   (min %.1f, max %.1f)" % ((k[:-3],) + tuple(res[k])))
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
