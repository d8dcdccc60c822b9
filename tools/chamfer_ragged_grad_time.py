"""Times the Chamfer backward over a ragged batch two ways: genpc_chamfer_backward_ragged (one call, ordered sums) and the
per-pair loop of genpc_chamfer_backward (B = 1 calls on slices of the same packed buffers, fp32 atomics into gradients zeroed
once per pass -- the only way before there was a ragged entry point).

Two batches:
  * waymo8: the first 8 Waymo car crops at their raw sizes against the complete car -- tests/golden/waymo_car59_4096.npz with
    every pad-repeated crop truncated to its count;
  * mix384: 384 synthetic pairs (the most one call takes), sizes drawn from 100 .. 600 (seeded).
Indices come from the ragged forward and the weights are seeded; inputs are packed and outputs allocated before the clock starts,
for both ways alike.  After a warm-up the two ways alternate; a repetition is `--inner` passes bracketed by HIP events on the
stream, reported per pass.  Median, 10th / 90th percentile and minimum of each, the ratio of the medians and the largest
difference between the two results go to profiles/chamfer_ragged_grad_time.json.  Needs a GPU.

    python tools/chamfer_ragged_grad_time.py [--reps 40] [--inner 10] [--warmup 5] [--out profiles/chamfer_ragged_grad_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def batches():
    z = np.load(os.path.join(ROOT, "tests", "golden", "waymo_car59_4096.npz"), allow_pickle=False)
    sizes = np.minimum(z["counts"][:8], 4096)
    waymo = [(np.ascontiguousarray(z["crops"][j, :sizes[j]]), np.ascontiguousarray(z["complete"])) for j in range(8)]
    rng = np.random.default_rng(384)
    mix = []
    for _ in range(384):
        n, m = (int(v) for v in rng.integers(100, 601, 2))
        c = rng.random((6, 3)) - 0.5
        a = (c[rng.integers(0, 6, n)] + 0.05 * rng.normal(size=(n, 3))).astype(np.float32)
        b = (c[rng.integers(0, 6, m)] + 0.05 * rng.normal(size=(m, 3))).astype(np.float32)
        mix.append((a, b))
    return {"waymo8": waymo, "mix384": mix}


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "p10_ms": float(np.percentile(a, 10)), "p90_ms": float(np.percentile(a, 90)),
            "min_ms": float(a[0]), "reps": int(len(a))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chamfer_ragged_grad_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("chamfer_ragged_grad_time: needs a GPU (a time taken elsewhere says nothing)")
    from genpc_amd import _lib, chamfer_3D
    dev = torch.device("cuda", torch.cuda.current_device())
    result = {"device": torch.cuda.get_device_name(dev), "inner": args.inner, "batches": {}}
    for name, pairs in batches().items():
        c = len(pairs)
        offa = [0] + [int(v) for v in np.cumsum([len(a) for a, _ in pairs])]
        offb = [0] + [int(v) for v in np.cumsum([len(b) for _, b in pairs])]
        PA = torch.from_numpy(np.concatenate([a for a, _ in pairs])).to(dev).contiguous()
        PB = torch.from_numpy(np.concatenate([b for _, b in pairs])).to(dev).contiguous()
        rng = np.random.default_rng(c)
        G1 = torch.from_numpy(rng.normal(size=offa[-1]).astype(np.float32)).to(dev)
        G2 = torch.from_numpy(rng.normal(size=offb[-1]).astype(np.float32)).to(dev)
        D1, D2 = torch.empty(offa[-1], device=dev), torch.empty(offb[-1], device=dev)
        I1, I2 = torch.empty(offa[-1], device=dev, dtype=torch.int32), torch.empty(offb[-1], device=dev, dtype=torch.int32)
        assert chamfer_3D.nm_distance_ragged(PA, offa, PB, offb, D1, I1) == 1, _lib.last_error()
        assert chamfer_3D.nm_distance_ragged(PB, offb, PA, offa, D2, I2) == 1, _lib.last_error()
        rg1, rg2 = torch.empty_like(PA), torch.empty_like(PB)
        lg1, lg2 = torch.empty_like(PA), torch.empty_like(PB)

        def cut(t, off):
            return [t[off[j]:off[j + 1]].unsqueeze(0) for j in range(c)]
        sl = [cut(PA, offa), cut(PB, offb), cut(lg1, offa), cut(lg2, offb), cut(G1, offa), cut(G2, offb), cut(I1, offa), cut(I2, offb)]

        def ragged():
            assert chamfer_3D.backward_ragged(PA, offa, PB, offb, rg1, rg2, G1, G2, I1, I2) == 1, _lib.last_error()

        def loop():
            lg1.zero_()
            lg2.zero_()
            for j in range(c):
                assert chamfer_3D.backward(*(s[j] for s in sl)) == 1, _lib.last_error()

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / args.inner

        for _ in range(args.warmup):
            ragged()
            loop()
        torch.cuda.synchronize()
        scale = max(float(lg1.abs().max()), float(lg2.abs().max()))
        diff = max(float((rg1 - lg1).abs().max()), float((rg2 - lg2).abs().max()))
        t_r, t_l = [], []
        for _ in range(args.reps):
            t_r.append(timed(ragged))
            t_l.append(timed(loop))
        r, l = stats(t_r), stats(t_l)
        result["batches"][name] = {"pairs": c, "points_a": offa[-1], "points_b": offb[-1],
                                   "sizes_a_min_max": [min(len(a) for a, _ in pairs), max(len(a) for a, _ in pairs)],
                                   "sizes_b_min_max": [min(len(b) for _, b in pairs), max(len(b) for _, b in pairs)],
                                   "max_abs_difference": diff, "max_abs_gradient": scale, "ragged": r, "loop": l,
                                   "loop_over_ragged": l["median_ms"] / r["median_ms"]}
        print(name, json.dumps(result["batches"][name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
