"""Times the auction EMD over a ragged batch three ways: ONE ragged call (genpc_emd_forward_ragged: 2 * iters + 2 launches
whatever the number of pairs), the Python loop of one emdModule call per pair (the only way before there was a ragged entry
point), and -- as context only, its result is another one -- the dense batched call on c clouds of max N_j points each.

Workloads (eps 0.005, 50 rounds):
  * a_64_mixed: 64 synthetic pairs, sizes cycling 256, 512 ... 4096;
  * b_13_large: 13 synthetic pairs, sizes cycling 8192, 9216 ... 16384;
  * c_13_scans: the 13 bundled partial-scan / ground-truth pairs (tests/golden/scans13_fps16384.npz), both sides of scan j
    farthest-point sampled to 2048 + 1024 j points.
Inputs are resident before the clock starts; each way allocates its own outputs inside the timed window, as a caller would.
The ragged call and the loop must give the same dist and assignment bits (asserted first).  After a warm-up the ways
alternate; each repetition is bracketed by HIP events on the stream.  Median, 10th / 90th percentile and minimum of each and
the ratio of the medians go to profiles/emd_ragged_time.json.  Needs a GPU; reads only tests/golden/.

    python tools/emd_ragged_time.py [--reps 20] [--warmup 3] [--out profiles/emd_ragged_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic(sizes, seed):
    rng = np.random.default_rng(seed)
    return [(rng.random((n, 3), dtype=np.float32), rng.random((n, 3), dtype=np.float32)) for n in sizes]


def scans(dev):
    from genpc_amd import fps
    z = np.load(os.path.join(ROOT, "tests", "golden", "scans13_fps16384.npz"), allow_pickle=False)
    part, gt = torch.from_numpy(z["partial"]).to(dev), torch.from_numpy(z["gt"]).to(dev)
    ks = [2048 + 1024 * j for j in range(part.shape[0])]
    out = []
    for j, k in enumerate(ks):
        ia, ib = fps.fps_sampling(part[j], k).long(), fps.fps_sampling(gt[j], k).long()
        out.append((part[j][ia].contiguous(), gt[j][ib].contiguous()))
    torch.cuda.synchronize()
    return out


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "p10_ms": float(np.percentile(a, 10)), "p90_ms": float(np.percentile(a, 90)),
            "min_ms": float(a[0]), "reps": int(len(a))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--eps", type=float, default=0.005)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "emd_ragged_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("emd_ragged_time: needs a GPU (a time taken elsewhere says nothing)")
    from genpc_amd.loss_functions import emdModule
    from genpc_amd.loss_functions.emd.emd_ragged import forward_packed
    dev = torch.device("cuda", torch.cuda.current_device())
    mod = emdModule()
    to_dev = lambda pairs: [(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)) for a, b in pairs]
    work = {"a_64_mixed": to_dev(synthetic([256 * (1 + j % 16) for j in range(64)], 64)),
            "b_13_large": to_dev(synthetic([8192 + 1024 * (j % 9) for j in range(13)], 13)),
            "c_13_scans": scans(dev)}
    result = {"device": torch.cuda.get_device_name(dev), "eps": args.eps, "iters": args.iters, "workloads": {}}
    for name, pairs in work.items():
        c = len(pairs)
        sizes = [int(a.shape[0]) for a, _ in pairs]
        off = [0] + [int(v) for v in np.cumsum(sizes)]
        PA, PB = torch.cat([a for a, _ in pairs]).contiguous(), torch.cat([b for _, b in pairs]).contiguous()
        singles = [(a[None].contiguous(), b[None].contiguous()) for a, b in pairs]
        nmax = max(sizes)
        # (the dense call's clouds are padded to max N_j with uniform random points: another problem, timed for scale only)
        gen = torch.Generator(device=dev).manual_seed(5)
        pad = lambda x: torch.cat([x, torch.rand((nmax - x.shape[0], 3), generator=gen, device=dev)])
        DA = torch.stack([pad(a) for a, _ in pairs]).contiguous()
        DB = torch.stack([pad(b) for _, b in pairs]).contiguous()
        keep = {}

        def ragged():
            s = forward_packed(PA, PB, off, args.eps, args.iters)
            keep["ragged"] = (s["dist"], s["assignment"])

        def loop():
            keep["loop"] = [mod(a, b, args.eps, args.iters) for a, b in singles]

        def dense():
            keep["dense"] = mod(DA, DB, args.eps, args.iters)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        for _ in range(args.warmup):
            ragged()
            loop()
            dense()
        torch.cuda.synchronize()
        same = (torch.equal(keep["ragged"][0].view(torch.int32), torch.cat([d[0] for d, _ in keep["loop"]]).view(torch.int32)) and
                torch.equal(keep["ragged"][1], torch.cat([i[0] for _, i in keep["loop"]])))
        assert same, "%s: the ragged call and the loop of emdModule calls differ" % name
        t = {"ragged": [], "loop": [], "dense": []}
        for _ in range(args.reps):
            t["ragged"].append(timed(ragged))
            t["loop"].append(timed(loop))
            t["dense"].append(timed(dense))
        r, l, d = stats(t["ragged"]), stats(t["loop"]), stats(t["dense"])
        result["workloads"][name] = {"pairs": c, "points": off[-1], "sizes_min_max": [min(sizes), max(sizes)], "same_bits": bool(same),
                                     "ragged": r, "loop": l, "dense_c_x_max_context_only": d,
                                     "loop_over_ragged": l["median_ms"] / r["median_ms"]}
        print(name, json.dumps(result["workloads"][name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
