"""Times the large farthest-point sampler (csrc/fps_large.hip, fps_sampling_large) beside the multi-workgroup kernel
(fps_sampling_multi, what clouds of 24577 to 262144 points take) at the sizes the pipeline samples, and alone at a million
points.  One process, warmed up, the two paths alternating call by call, the device synchronised round every call; the
figures are wall time of the whole call (grid build, sampling, in-line check, the host's read of the first indices).

    python tools/fps_large_time.py [--reps 7] [--only-large]

--only-large runs the million-point case alone (for a kernel trace that states the sampling and its check separately).
DESIGN.md 4.6 records what this printed."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from genpc_amd import _lib, fps  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "runs": len(ms)}


def rounds_of(x, c):
    r = (ctypes.c_int * c)()
    _lib.on_device_of(x, _lib.lib.genpc_fps_stats, c, ctypes.addressof(r))
    return list(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only-large", action="store_true")
    a = ap.parse_args()
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    res = {}
    if not a.only_large:
        for c, n, k in ((4, 165546, 16384), (1, 185000, 20000), (16, 185000, 20000)):
            clouds = [torch.rand(n, 3, device="cuda", generator=g) for _ in range(c)]
            ks = [k] * c
            paths = {"large": lambda: fps.fps_sampling_large(clouds, ks), "multi_workgroup": lambda: fps.fps_sampling_multi(clouds, ks)}
            ms = {name: [] for name in paths}
            outs = {}
            for name, fn in paths.items():
                fn()
            for _ in range(a.reps):
                for name, fn in paths.items():
                    dt, outs[name] = timed(fn)
                    ms[name].append(dt)
            same = all(torch.equal(x, y) for x, y in zip(outs["large"], outs["multi_workgroup"]))
            res["%dx%d->%d" % (c, n, k)] = {"same_sequences": same, **{name: summary(v) for name, v in ms.items()}}
            print(json.dumps({"%dx%d->%d" % (c, n, k): res["%dx%d->%d" % (c, n, k)]}), flush=True)
    n, k = 1000000, 16384
    cloud = torch.rand(n, 3, device="cuda", generator=g)
    fps.fps_sampling(cloud, 64)
    ms = []
    for _ in range(max(3, a.reps // 2)):
        dt, _ = timed(lambda: fps.fps_sampling(cloud, k))
        ms.append(dt)
    r = rounds_of(cloud, 1)[0]
    res["1x%d->%d" % (n, k)] = {"large": summary(ms), "rounds": r, "samples_per_round": round(k / max(1, r), 1)}
    print(json.dumps({"1x%d->%d" % (n, k): res["1x%d->%d" % (n, k)]}), flush=True)
    print(json.dumps({"fps_large_time": res, "stats": fps.stats}))


if __name__ == "__main__":
    main()
