"""Times the surface sampling of a mesh of about 2 * 10^5 faces, 163 840 samples with colours, resident on the device at
the end, three ways:

  host      the host sampler's arrays (utils/mesh_io._glb2point_full: numpy areas, cumsum, searchsorted, gathers, the
            barycentric solve) plus their upload as float32 -- what reg() does without a seed;
  upload    sample_surface_gpu from host arrays (conversion to float32 / int32, one upload, the kernels);
  resident  sample_surface_gpu from arrays already on the device;
  kernels   the library call alone in a loop on preallocated buffers, between device events: the memset and the four
            launches per call, back to back (the larger of their device time and the host's enqueue time).

Each figure is the median of --repeats runs after --warmup, a host clock around work that ends in a device synchronise
(device events for the last).  Nothing is asserted.

    python tools/mesh_sample_time.py [--freq 100] [--samples 163840] [--repeats 20] [--json OUT]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def icosphere(freq, seed=0, jitter=0.15):
    """A sphere of 20 * freq^2 triangles (every icosahedron face cut freq ways along an edge), vertices jittered along and
    across the surface by `jitter` of an edge length, with vertex colours -> (V float64, F int64, C float64)."""
    t = (1 + 5 ** 0.5) / 2
    P = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], np.float64)
    T = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    verts, faces = [], []
    for a, b, c in T:
        base = sum(len(v) for v in verts)
        index = {}
        pts = []
        for i in range(freq + 1):
            for j in range(freq + 1 - i):
                index[(i, j)] = base + len(pts)
                pts.append((P[a] * (freq - i - j) + P[b] * i + P[c] * j) / freq)
        verts.append(np.array(pts))
        for i in range(freq):
            for j in range(freq - i):
                faces.append((index[(i, j)], index[(i + 1, j)], index[(i, j + 1)]))
                if i + j < freq - 1:
                    faces.append((index[(i + 1, j)], index[(i + 1, j + 1)], index[(i, j + 1)]))
    V = np.concatenate(verts)
    V /= np.linalg.norm(V, axis=1, keepdims=True)
    # weld the vertices the 20 patches share
    _, first, inverse = np.unique(np.round(V * 1e6).astype(np.int64), axis=0, return_index=True, return_inverse=True)
    V, F = V[first], inverse.reshape(-1)[np.array(faces, np.int64)]
    rng = np.random.default_rng(seed)
    V = V + jitter * (4.0 / (freq * 2.0)) * rng.standard_normal(V.shape)
    C = rng.random(V.shape)
    return V.astype(np.float32).astype(np.float64), F, C.astype(np.float32).astype(np.float64)


def median_ms(fn, warmup, repeats, sync):
    for _ in range(warmup):
        fn()
    sync()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--freq", type=int, default=100, help="20 * freq^2 faces")
    ap.add_argument("--samples", type=int, default=163840)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--loop", type=int, default=200, help="library calls between the two device events")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    from genpc_amd import _lib
    from genpc_amd.utils import mesh_io as M
    if not torch.cuda.is_available():
        raise SystemExit("mesh_sample_time: needs a GPU (a CPU run times nothing of interest)")
    dev = torch.device("cuda", torch.cuda.current_device())
    V, F, C = icosphere(args.freq)
    n = args.samples
    res = {"faces": int(len(F)), "vertices": int(len(V)), "samples": n, "device": torch.cuda.get_device_name(dev)}
    sync = torch.cuda.synchronize

    # host: _glb2point_full on these arrays (the file parsing is not part of any of the three paths)
    load = M.load_glb
    M.load_glb = lambda path: (V, F, C)
    try:
        rng = np.random.default_rng(0)

        def host():
            pts, col = M._glb2point_full("mesh.glb", n, rng)
            return torch.as_tensor(pts, dtype=torch.float32, device=dev), torch.as_tensor(col, dtype=torch.float32, device=dev)
        res["host_ms"] = median_ms(host, 2, max(5, args.repeats // 2), sync)
    finally:
        M.load_glb = load
    res["upload_ms"] = median_ms(lambda: M.sample_surface_gpu(V, F, n, 1, colors=C, device=dev), args.warmup, args.repeats, sync)
    Vd, Fd, Cd = [M._device_array(a, t, dev, "x") for a, t in ((V, torch.float32), (F, torch.int32), (C, torch.float32))]
    res["resident_ms"] = median_ms(lambda: M.sample_surface_gpu(Vd, Fd, n, 1, colors=Cd), args.warmup, args.repeats, sync)

    # the library call alone, preallocated, between device events
    L, p = _lib.lib, _lib.ptr
    ws = torch.empty(L.genpc_mesh_sample_bytes(len(F)), dtype=torch.uint8, device=dev)
    pts, col = torch.empty(n, 3, device=dev), torch.empty(n, 3, device=dev)
    fi, st = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)

    def call():
        return _lib.on_device_of(Vd, L.genpc_mesh_sample, len(V), p(Vd), p(Cd), len(F), p(Fd), n, 1, p(pts), p(col), p(fi), p(None),
                                 p(st), p(ws))
    for _ in range(20):
        assert call() == 1
    sync()
    per_call = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.loop):
            call()
        e1.record()
        e1.synchronize()
        per_call.append(e0.elapsed_time(e1) / args.loop * 1e3)
    per_call.sort()
    res["kernels_us_per_call"] = (per_call[len(per_call) // 2], per_call[0], per_call[-1])
    assert int(st.item()) == 1
    for k in ("host_ms", "upload_ms", "resident_ms"):
        print("%-12s median %9.3f ms   (min %.3f, max %.3f)" % ((k[:-3],) + tuple(res[k])))
    print("%-12s median %9.1f us per call (min %.1f, max %.1f; %d calls between events)" % (("kernels",) + tuple(res["kernels_us_per_call"]) + (args.loop,)))
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
