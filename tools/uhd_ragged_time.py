"""Times the directed Hausdorff distance over a ragged batch two ways: genpc_uhd_ragged (one call, four launches) and the
per-pair loop of genpc_uhd (B = 1 calls of three launches each, the only way before there was a ragged entry point).

Two batches:
  * waymo59: the 59 Waymo car crops at their raw sizes (queries) against the complete car (targets) --
    tests/golden/waymo_car59_4096.npz as tools/nn_ragged_time.py loads it, every pad-repeated crop truncated to its count (a
    crop the fixture subsampled stays at 4096);
  * mix64: 64 synthetic pairs, sizes drawn from 100 .. 8192 (seeded).
Inputs are packed and outputs allocated before the clock starts, for both ways alike.  Both ways must give the same bits
(asserted first).  After a warm-up the two ways alternate; each repetition is bracketed by HIP events on the stream.  Median,
10th / 90th percentile and minimum of each, and the ratio of the medians, go to profiles/uhd_ragged_time.json.  Needs a GPU;
reads only tests/golden/.

    python tools/uhd_ragged_time.py [--reps 40] [--warmup 5] [--out profiles/uhd_ragged_time.json]
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


def batches():
    z = np.load(os.path.join(ROOT, "tests", "golden", "waymo_car59_4096.npz"), allow_pickle=False)
    car = np.ascontiguousarray(z["complete"])
    sizes = np.minimum(z["counts"], 4096)
    waymo = [(np.ascontiguousarray(z["crops"][j, :sizes[j]]), car) for j in range(len(sizes))]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uhd_ragged_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("uhd_ragged_time: needs a GPU (a time taken elsewhere says nothing)")
    from genpc_amd import _lib
    lib = _lib.lib
    dev = torch.device("cuda", torch.cuda.current_device())
    result = {"device": torch.cuda.get_device_name(dev), "batches": {}}
    for name, pairs in batches().items():
        c = len(pairs)
        A = [torch.from_numpy(a).to(dev) for a, _ in pairs]
        B = [torch.from_numpy(b).to(dev) for _, b in pairs]
        offa = [0] + [int(v) for v in np.cumsum([len(a) for a in A])]
        offb = [0] + [int(v) for v in np.cumsum([len(b) for b in B])]
        PA, PB = torch.cat(A).contiguous(), torch.cat(B).contiguous()
        na, nb = (ctypes.c_int * (c + 1))(*offa), (ctypes.c_int * (c + 1))(*offb)
        pna, pnb = ctypes.cast(na, ctypes.c_void_p), ctypes.cast(nb, ctypes.c_void_p)
        rd, ri = torch.empty(c, dtype=torch.float64, device=dev), torch.empty((c, 2), dtype=torch.int32, device=dev)
        ld, li = torch.empty_like(rd), torch.empty_like(ri)
        lptr = [(len(A[j]), A[j].data_ptr(), len(B[j]), B[j].data_ptr(), ld[j:].data_ptr(), li[j:].data_ptr()) for j in range(c)]
        stream = _lib.stream_of(PA)

        def ragged():
            assert lib.genpc_uhd_ragged(c, pna, PA.data_ptr(), pnb, PB.data_ptr(), rd.data_ptr(), ri.data_ptr(), stream) == 0, _lib.last_error()

        def loop():
            for n, a, m, b, d, i in lptr:
                assert lib.genpc_uhd(1, n, a, m, b, d, i, stream) == 0, _lib.last_error()

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
        same = torch.equal(rd.view(torch.int64), ld.view(torch.int64)) and torch.equal(ri, li)
        assert same, "%s: the ragged call and the loop of genpc_uhd differ" % name
        t_r, t_l = [], []
        for _ in range(args.reps):
            t_r.append(timed(ragged))
            t_l.append(timed(loop))
        r, l = stats(t_r), stats(t_l)
        result["batches"][name] = {"pairs": c, "queries": offa[-1], "targets": offb[-1],
                                   "query_sizes_min_max": [min(len(a) for a in A), max(len(a) for a in A)],
                                   "target_sizes_min_max": [min(len(b) for b in B), max(len(b) for b in B)],
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
