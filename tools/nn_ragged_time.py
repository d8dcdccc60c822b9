"""Times both Chamfer directions over a ragged batch two ways: genpc_nm_distance_ragged (one call per direction) and the
per-pair loop of genpc_nm_distance (B = 1 calls, the only way before there was a ragged entry point).

Two batches:
  * waymo59: the 59 Waymo car crops at their raw sizes against the complete car -- tests/golden/waymo_car59_4096.npz with every
    pad-repeated crop truncated to its count (a crop the fixture subsampled stays at 4096);
  * mix64: 64 synthetic pairs, sizes drawn from 100 .. 8192 (seeded).
Inputs are packed and outputs allocated before the clock starts, for both ways alike.  After a warm-up the two ways
alternate; each repetition is bracketed by HIP events on the stream.  Median, 10th / 90th percentile and minimum of
each, and the ratio of the medians, go to profiles/nn_ragged_time.json.  Needs a GPU.

    python tools/nn_ragged_time.py [--reps 40] [--warmup 5] [--out profiles/nn_ragged_time.json]
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
    sizes = np.minimum(z["counts"], 4096)
    waymo = [(np.ascontiguousarray(z["crops"][j, :sizes[j]]), np.ascontiguousarray(z["complete"])) for j in range(len(sizes))]
    rng = np.random.default_rng(64)
    mix = []
    for _ in range(64):
        n, m = (int(v) for v in rng.integers(100, 8193, 2))
        c = rng.random((6, 3)) - 0.5
        a = (c[rng.integers(0, 6, n)] + 0.05 * rng.normal(size=(n, 3))).astype(np.float32)
        b = (c[rng.integers(0, 6, m)] + 0.05 * rng.normal(size=(m, 3))).astype(np.float32)
        mix.append((a, b))
    return {"waymo59": waymo, "mix64": mix}


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "p10_ms": float(np.percentile(a, 10)), "p90_ms": float(np.percentile(a, 90)),
            "min_ms": float(a[0]), "reps": int(len(a))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nn_ragged_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nn_ragged_time: needs a GPU (a time taken elsewhere says nothing)")
    from genpc_amd import _lib, chamfer_3D
    dev = torch.device("cuda", torch.cuda.current_device())
    result = {"device": torch.cuda.get_device_name(dev), "arith_mode": _lib.lib.genpc_get_arith(), "batches": {}}
    for name, pairs in batches().items():
        A = [torch.from_numpy(a).to(dev) for a, _ in pairs]
        B = [torch.from_numpy(b).to(dev) for _, b in pairs]
        offa = [0] + list(np.cumsum([len(a) for a in A]))
        offb = [0] + list(np.cumsum([len(b) for b in B]))
        PA, PB = torch.cat(A).contiguous(), torch.cat(B).contiguous()
        rd = [torch.empty(PA.shape[0], device=dev), torch.empty(PB.shape[0], device=dev)]
        ri = [torch.empty(PA.shape[0], device=dev, dtype=torch.int32), torch.empty(PB.shape[0], device=dev, dtype=torch.int32)]
        A1, B1 = [a.unsqueeze(0) for a in A], [b.unsqueeze(0) for b in B]
        ld = [torch.empty_like(rd[0]), torch.empty_like(rd[1])]
        li = [torch.empty_like(ri[0]), torch.empty_like(ri[1])]
        lda = [ld[0][offa[j]:offa[j + 1]].unsqueeze(0) for j in range(len(pairs))]
        lia = [li[0][offa[j]:offa[j + 1]].unsqueeze(0) for j in range(len(pairs))]
        ldb = [ld[1][offb[j]:offb[j + 1]].unsqueeze(0) for j in range(len(pairs))]
        lib_ = [li[1][offb[j]:offb[j + 1]].unsqueeze(0) for j in range(len(pairs))]

        def ragged():
            assert chamfer_3D.nm_distance_ragged(PA, offa, PB, offb, rd[0], ri[0]) == 1, _lib.last_error()
            assert chamfer_3D.nm_distance_ragged(PB, offb, PA, offa, rd[1], ri[1]) == 1, _lib.last_error()

        def loop():
            for j in range(len(pairs)):
                assert chamfer_3D.nm_distance(A1[j], B1[j], lda[j], lia[j]) == 1, _lib.last_error()
                assert chamfer_3D.nm_distance(B1[j], A1[j], ldb[j], lib_[j]) == 1, _lib.last_error()

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
        torch.cuda.synchronize()
        same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(rd + ri, ld + li))
        t_r, t_l = [], []
        for _ in range(args.reps):
            t_r.append(timed(ragged))
            t_l.append(timed(loop))
        r, l = stats(t_r), stats(t_l)
        result["batches"][name] = {"pairs": len(pairs), "points_a": int(offa[-1]), "points_b": int(offb[-1]),
                                   "sizes_a_min_max": [int(min(len(a) for a in A)), int(max(len(a) for a in A))],
                                   "sizes_b_min_max": [int(min(len(b) for b in B)), int(max(len(b) for b in B))],
                                   "same_bits": bool(same), "ragged": r, "loop": l,
                                   "loop_over_ragged": l["median_ms"] / r["median_ms"]}
        print(name, json.dumps(result["batches"][name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
