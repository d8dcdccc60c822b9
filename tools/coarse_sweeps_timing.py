"""Times the stage of reg() between the pose initialisation and the fusion tail over S scans two ways: the loop, per scan, of
reg_xyz.voxel_down_sample x 2 + reg_xyz.coarse_scale_sweep (per scan: two voxel calls of seven launches and two rocprim
primitives each, ending in a count read-back, and two genpc_icp_batch calls with a copy back after each) and the ragged forms,
reg_xyz.voxel_down_sample_clouds + reg_xyz.coarse_scale_sweeps (one voxel call and one read-back, two ICP calls of one launch and
one copy back each, the Chamfer scores through chamfer_ragged) -- whatever S is.

The shape is reg()'s own: S = 1, 4 and 16 scans, each two seeded samplings of a box's surface (20000 raw points a side) that a
0.03 voxel grid brings to about 3000 + 3000 points; the source is 1.08 times smaller, turned by 3 degrees and moved.  Both ways
must find the same best scale and coarse transformation (asserted first).  After a warm-up the ways alternate, in an order that
reverses every repetition; each repetition is bracketed by HIP events on the stream.  The two stages are also timed alone.

--baseline-lib PATH: another build of libgenpc_hip.so (the commit before this one), loaded beside this one: genpc_icp_batch with
the sweep's 11 candidates on scan 0's clouds runs through both, interleaved in the same process -- how a time at one commit is
compared with a time at another (the one-workgroup kernel's body moved into a device function; its time must not have).

Median, 10th / 90th percentile and minimum of each go to profiles/coarse_sweeps_time.json.  Needs a GPU.

    python tools/coarse_sweeps_timing.py [--reps 30] [--warmup 5] [--sizes 1,4,16] [--baseline-lib PATH] [--out profiles/coarse_sweeps_time.json]
"""
import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RAW = 20000
VOXEL = 0.03
HALF = np.array([0.5, 0.3, 0.2])


def rot(axis, deg):
    a = np.asarray(axis, float)
    a /= np.linalg.norm(a)
    th = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def box_surface(seed, n):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1.0, 1.0, (n, 3))
    axis = rng.integers(0, 3, n)
    p[np.arange(n), axis] = rng.choice([-1.0, 1.0], n)
    return p * HALF


def scan(seed):
    tgt = box_surface(seed, RAW).astype(np.float32)
    Rm, t = rot([0.1, 1.0, 0.3], 3.0), np.array([0.01, -0.012, 0.008])
    src = ((box_surface(seed + 500, RAW) / 1.08 - t) @ Rm).astype(np.float32)
    return src, tgt


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "p10_ms": float(np.percentile(a, 10)), "p90_ms": float(np.percentile(a, 90)),
            "min_ms": float(a[0]), "reps": int(len(a))}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns, reps):
    """Every way once per repetition, the order reversed every other repetition."""
    t = {name: [] for name in fns}
    names = list(fns)
    for r in range(reps):
        for name in (names if r % 2 == 0 else names[::-1]):
            t[name].append(timed(fns[name]))
    return {name: stats(v) for name, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="1,4,16")
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coarse_sweeps_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("coarse_sweeps_timing: needs a GPU (a time taken elsewhere says nothing)")
    if args.reps < 20:
        raise SystemExit("coarse_sweeps_timing: at least 20 repetitions")
    from genpc_amd import _lib, reg_xyz
    dev = torch.device("cuda", torch.cuda.current_device())
    sizes = [int(v) for v in args.sizes.split(",")]
    raw = [tuple(torch.from_numpy(c).to(dev) for c in scan(100 + j)) for j in range(max(sizes))]
    result = {"device": torch.cuda.get_device_name(dev), "raw_points_per_cloud": RAW, "voxel": VOXEL, "scales": 11,
              "baseline_lib": bool(args.baseline_lib), "batches": {}}

    def loop_voxel(scans):
        return [(reg_xyz.voxel_down_sample(s, VOXEL), reg_xyz.voxel_down_sample(t, VOXEL)) for s, t in scans]

    def ragged_voxel(scans):
        down = reg_xyz.voxel_down_sample_clouds([c for pair in scans for c in pair], VOXEL)
        return down[0::2], down[1::2]

    for s in sizes:
        scans = raw[:s]
        fns = {"loop": lambda: [reg_xyz.coarse_scale_sweep(a, b) for a, b in loop_voxel(scans)],
               "ragged": lambda: reg_xyz.coarse_scale_sweeps(*ragged_voxel(scans))}
        down = loop_voxel(scans)
        src, tgt = [d[0] for d in down], [d[1] for d in down]
        stage = {"voxel_loop": lambda: loop_voxel(scans), "voxel_ragged": lambda: ragged_voxel(scans),
                 "sweep_loop": lambda: [reg_xyz.coarse_scale_sweep(a, b) for a, b in zip(src, tgt)],
                 "sweep_ragged": lambda: reg_xyz.coarse_scale_sweeps(src, tgt)}
        got = {}
        for _ in range(args.warmup):
            for name, fn in list(fns.items()) + list(stage.items()):
                got[name] = fn()
        torch.cuda.synchronize()
        for a, b in zip(got["loop"], got["ragged"]):
            assert a[0] == b[0] and np.array_equal(a[2], b[2]), "S=%d: the two ways disagree" % s
        row = alternate(fns, args.reps)
        row.update(alternate(stage, args.reps))
        for name in row:
            row[name]["per_scan_ms"] = row[name]["median_ms"] / s
        row["points_after_grid"] = [[int(a.shape[0]), int(b.shape[0])] for a, b in zip(src, tgt)]
        row["loop_over_ragged"] = row["loop"]["median_ms"] / row["ragged"]["median_ms"]
        result["batches"]["S%d" % s] = row
        print("S=%d" % s, json.dumps(row), flush=True)

    if args.baseline_lib:
        base = ctypes.CDLL(os.path.abspath(args.baseline_lib))
        sig = _lib.SIGNATURES["genpc_icp_batch"]
        base.genpc_icp_batch.restype, base.genpc_icp_batch.argtypes = sig
        src, tgt = reg_xyz.voxel_down_sample(raw[0][0], VOXEL), reg_xyz.voxel_down_sample(raw[0][1], VOXEL)
        inits = []
        for sc in np.linspace(1.5, 0.8, 11):
            S = np.eye(4)
            S[:3, :3] *= sc
            inits.append(S)
        init = torch.as_tensor(np.stack(inits).reshape(11, 16)).contiguous().to(dev)
        outs = {w: (torch.empty(11, 16, dtype=torch.float64, device=dev), torch.empty(11, 3, dtype=torch.float64, device=dev)) for w in ("this", "baseline")}

        def icp(lib, w):
            assert lib.genpc_icp_batch(11, src.shape[0], src.data_ptr(), tgt.shape[0], tgt.data_ptr(), 0.075, init.data_ptr(), 30, 1e-6, 1e-6,
                                       outs[w][0].data_ptr(), outs[w][1].data_ptr(), _lib.stream_of(src)) == 1

        fns = {"this": lambda: icp(_lib.lib, "this"), "baseline": lambda: icp(base, "baseline")}
        for _ in range(args.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        assert torch.equal(outs["this"][0], outs["baseline"][0]) and torch.equal(outs["this"][1], outs["baseline"][1]), "the kernel's results moved"
        row = alternate(fns, args.reps * 3)
        row["this_over_baseline"] = row["this"]["median_ms"] / row["baseline"]["median_ms"]
        row["points"] = [int(src.shape[0]), int(tgt.shape[0])]
        result["icp_batch_11_candidates"] = row
        print("icp_batch x11", json.dumps(row), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
