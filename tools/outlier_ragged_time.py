"""Times the statistical outlier filter over S clouds two ways: reg_xyz.remove_noise_from_point_clouds (one library call:
three launches whatever S is, statistics and mask on the device) and the loop of reg_xyz.remove_noise_from_point_cloud over
the same clouds (per cloud: genpc_knn_mean_distance's two launches, then torch's reductions and compare, and a boolean index
that waits for the device) -- the only way before there was a ragged entry point.

The shape is fuse's own: S = 1, 4, 16 and 64 clouds of 20000 points, k = 20, std_ratio 2.5.  Two kinds of cloud (seeded, made
before the clock starts): `surface`, an ellipsoid's surface with 2 % of its points displaced off it -- what a fused scan looks
like, and the displaced points are the lanes that walk far: the search's long tail -- and `uniform`, points uniform in a cube,
where every lane finds its neighbours in the first shells.  Both ways must keep the same points (asserted first).  After a
warm-up the ways alternate, in an order that reverses every repetition; each repetition is bracketed by HIP events on the
stream.  Also timed, on ONE cloud, the single library call genpc_knn_mean_distance alone.

--baseline-lib PATH: another build of libgenpc_hip.so (the commit before the ragged filter), loaded beside this one; the single
call runs through both, and so does the body of remove_noise_from_point_cloud, restated here with the library as a parameter
(`loop_body`, `loop_body_baseline`), all interleaved in the same process, which is how a time at one commit is compared with
a time at another.

Median, 10th / 90th percentile and minimum of each go to profiles/outlier_ragged_time.json.  Needs a GPU.

    python tools/outlier_ragged_time.py [--reps 30] [--warmup 5] [--baseline-lib PATH] [--out profiles/outlier_ragged_time.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POINTS = 20000
K = 20
RATIO = 2.5


def cloud(kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.random((POINTS, 3), dtype=np.float32) - np.float32(0.5)
    v = rng.standard_normal((POINTS, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    p = (v * np.array([0.5, 0.3, 0.2])).astype(np.float32)
    k = POINTS // 50
    p[:k] += (0.3 * rng.standard_normal((k, 3))).astype(np.float32)
    return p


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="1,4,16,64")
    ap.add_argument("--kinds", default="surface,uniform")
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outlier_ragged_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("outlier_ragged_time: needs a GPU (a time taken elsewhere says nothing)")
    from genpc_amd import _lib, reg_xyz
    dev = torch.device("cuda", torch.cuda.current_device())
    base = None
    if args.baseline_lib:
        base = ctypes.CDLL(os.path.abspath(args.baseline_lib))
        base.genpc_knn_mean_distance.restype = ctypes.c_int
        base.genpc_knn_mean_distance.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]

    def single(lib, pts, out):
        assert lib.genpc_knn_mean_distance(POINTS, pts.data_ptr(), K, out.data_ptr(), _lib.stream_of(pts)) == 1

    def noise_loop(lib, clouds, out):
        """reg_xyz.remove_noise_from_point_cloud's body per cloud, with `lib`'s genpc_knn_mean_distance."""
        res = []
        for pts in clouds:
            single(lib, pts, out)
            m = out.double()
            mean = m.mean()
            std = torch.sqrt(((m - mean) ** 2).sum() / (m.numel() - 1))
            keep = m < mean + RATIO * std
            res.append((pts[keep], keep))
        return res

    sizes = [int(v) for v in args.sizes.split(",")]
    out = torch.empty(POINTS, device=dev)
    ways = {"this": _lib.lib}
    if base is not None:
        ways["baseline"] = base
    result = {"device": torch.cuda.get_device_name(dev), "points_per_cloud": POINTS, "k": K, "std_ratio": RATIO,
              "baseline_lib": bool(base), "launches": {"ragged_call": 3, "loop_per_cloud_library": 2}, "kinds": {}}

    def alternate(fns, reps):
        """Every way once per repetition, the order reversed every other repetition."""
        t = {name: [] for name in fns}
        names = list(fns)
        for r in range(reps):
            for name in (names if r % 2 == 0 else names[::-1]):
                t[name].append(timed(fns[name]))
        return {name: stats(v) for name, v in t.items()}

    for kind in args.kinds.split(","):
        all_clouds = [torch.from_numpy(cloud(kind, 1000 + j)).to(dev) for j in range(max(sizes))]
        res = {"single_call": {}, "batches": {}}
        singles = {w: (lambda lib=lib: single(lib, all_clouds[0], out)) for w, lib in ways.items()}
        for _ in range(args.warmup):
            for fn in singles.values():
                fn()
        torch.cuda.synchronize()
        res["single_call"] = alternate(singles, args.reps * 3)
        print(kind, "single_call", json.dumps(res["single_call"]), flush=True)
        for s in sizes:
            clouds = all_clouds[:s]
            packed = (torch.cat(clouds).contiguous(), [POINTS * j for j in range(s + 1)])
            fns = {"ragged": lambda: reg_xyz.remove_noise_from_point_clouds(packed, nb_neighbors=K, std_ratio=RATIO),
                   "loop": lambda: [reg_xyz.remove_noise_from_point_cloud(c, nb_neighbors=K, std_ratio=RATIO) for c in clouds]}
            if base is not None:          # (the same body through both libraries: remove_noise_from_point_cloud itself checks and allocates more)
                fns["loop_body"] = lambda: noise_loop(_lib.lib, clouds, out)
                fns["loop_body_baseline"] = lambda: noise_loop(base, clouds, out)
            got = {}
            for _ in range(args.warmup):
                for name, fn in fns.items():
                    got[name] = fn()
            torch.cuda.synchronize()
            for name in fns:
                if name != "ragged":
                    assert all(torch.equal(a, b[1]) for a, b in zip(got["ragged"][1], got[name])), "%s S=%d: %s keeps other points" % (kind, s, name)
            row = alternate(fns, args.reps)
            for name in fns:
                row[name]["per_cloud_ms"] = row[name]["median_ms"] / s
            row["loop_over_ragged"] = row["loop"]["median_ms"] / row["ragged"]["median_ms"]
            res["batches"]["S%d" % s] = row
            print(kind, "S=%d" % s, json.dumps(row), flush=True)
        result["kinds"][kind] = res
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
