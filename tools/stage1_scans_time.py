"""Times the batched stage 1 and the batched chain against what they stand beside, both sides in the same process, alternating:

  (a) stage 1   DepthPrompting.getDepths + ScaleAdapter.colorPoints over S scans of N points against the loop of getDepth +
                colorPoint, at the pipeline's default cfg (1024 views, res 256); and the part after hidden-point removal
                alone: one genpc_depth_prompt_ragged call between device events.
  (b) chain     pipeline.complete_scans_batched against pipeline.complete_scans(lanes=6) on S jobs (--chain-repeats runs).

Each figure is the median of --repeats runs after --warmup with the smallest and the largest, a host clock around work that
ends in a device synchronise.  Nothing is asserted but that the two sides of (a) return the same bits.

    python tools/stage1_scans_time.py [--scans 16] [--points 8192] [--repeats 20] [--json OUT]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


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


def shell(seed, n, scale=1.0):
    """A bumped half ellipsoid: an observed scan with a front and a back."""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    p[:, 2] = np.abs(p[:, 2])
    return (p * np.array([0.45, 0.3, 0.25]) * scale * (1 + 0.01 * rng.normal(size=(n, 1)))).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=16)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--chain-repeats", type=int, default=5)
    ap.add_argument("--no-chain", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    from genpc_amd import pipeline
    from genpc_amd.DepthPrompting import DepthPrompting
    from genpc_amd.ScaleAdapter import ScaleAdapter
    if not torch.cuda.is_available():
        raise SystemExit("stage1_scans_time: needs a GPU (a CPU run times nothing of interest)")
    dev = torch.device("cuda", torch.cuda.current_device())
    sync = torch.cuda.synchronize
    s, n = args.scans, args.points
    cfg = pipeline.default_cfg(dev)
    dp, sa = DepthPrompting(cfg), ScaleAdapter(cfg)
    res = {"scans": s, "points": n, "device": torch.cuda.get_device_name(dev), "repeats": args.repeats}
    clouds = [torch.from_numpy(shell(40 + j, n - 37 * j)).to(dev) for j in range(s)]
    g = torch.Generator().manual_seed(1)
    imgs = torch.rand(s, 3, 1024, 1024, generator=g).to(dev)

    def batched():
        gs = dp.getDepths(clouds)
        return gs, sa.colorPoints([x["uv"] for x in gs], imgs)

    def loop():
        gs = [dp.getDepth(c) for c in clouds]
        return gs, [sa.colorPoint(x["uv"], imgs[j]) for j, x in enumerate(gs)]
    (ga, ca), (gb, cb) = batched(), loop()
    for j in range(s):
        assert ga[j]["view_index"] == gb[j]["view_index"] and ga[j]["used_opposite"] == gb[j]["used_opposite"], j
        assert all(torch.equal(ga[j][k], gb[j][k]) for k in ("uv", "pixels", "visible", "sparse_img", "raw_depth", "hole_mask1", "hole_mask2")), j
        assert torch.equal(ca[j], cb[j]), j
    res["stage1_batched_ms"], res["stage1_loop_ms"] = alternate([batched, loop], args.warmup, args.repeats, sync)

    # the part after hidden-point removal alone, between device events: the one call on the batch's own masks
    import ctypes
    from genpc_amd import _lib
    L, p = _lib.lib, _lib.ptr
    off = [0]
    for c in clouds:
        off.append(off[-1] + c.shape[0])
    T = off[-1]
    xyz, rgb = torch.cat(clouds).contiguous(), torch.ones(T, 3, device=dev)
    cams = torch.stack([torch.stack([dp.cams[j], dp.cams[j]]) for j in range(s)]).contiguous()
    vis = torch.cat([torch.stack([x["visible"], x["visible"]]).to(torch.uint8).reshape(-1) for x in ga]).contiguous()
    R = cfg.res
    outs = [torch.empty(T, 2, device=dev), torch.empty(T, device=dev), torch.empty(T, 2, device=dev, dtype=torch.int32),
            torch.empty(T, device=dev, dtype=torch.uint8), torch.empty(s, device=dev, dtype=torch.int32),
            torch.empty(s, 2, device=dev, dtype=torch.float64), torch.empty(s, 4, 3, R, R, device=dev), torch.empty(s, device=dev, dtype=torch.int32)]
    harr = (ctypes.c_int * (s + 1))(*off)

    def call():
        return _lib.on_device_of(xyz, L.genpc_depth_prompt_ragged, s, ctypes.cast(harr, ctypes.c_void_p), p(xyz), p(rgb), p(cams), p(vis),
                                 float(dp.focal), 1e-2, 1e2, 1, float(np.float32(1 - 2 * cfg.padding)), R, cfg.point_size, cfg.mask_pixel_rate,
                                 *[p(t) for t in outs])
    for _ in range(3):
        assert call() == 1
    sync()
    per = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            call()
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) / 10 * 1e3)
    per.sort()
    res["depth_prompt_ragged_us"] = (per[len(per) // 2], per[0], per[-1])
    assert outs[7].tolist() == [1] * s

    if not args.no_chain:
        jobs = []
        for j in range(s):
            gen = torch.from_numpy(np.concatenate([shell(140 + j, 12000, 1.15), shell(240 + j, 8000, 1.15) * np.float32([1, 1, -1])])).to(dev)
            jobs.append((clouds[j], gen, imgs[j], torch.from_numpy(shell(340 + j, 16384)).to(dev)))
        dps = [DepthPrompting(cfg) for _ in range(6)]
        fns = [lambda: pipeline.complete_scans_batched(jobs, cfg=cfg, dp=dp), lambda: pipeline.complete_scans(jobs, lanes=6, cfg=cfg, dps=dps)]
        res["chain_batched_ms"], res["chain_lanes6_ms"] = alternate(fns, 1, args.chain_repeats, sync)
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
