"""Times the k-nearest-neighbour query of S scans two ways: one knn.knn_query_ragged call (genpc_knn_query_ragged: three
launches and one workspace layout whatever S is) and the loop of S knn.knn_query calls on the same data (three launches and
one workspace layout each) -- the only way before there was a ragged entry point.

The shape is stage 1's densification: S = 16 pairs, 5000 queries each (the reference's add_num_points) drawn uniformly in
the bounding box of the pair's targets, as generate_interpolation_points draws them; the targets are clustered clouds (five
centres, sigma 0.02: tests/test_gpu_knn_query.py's `clustered`) of 2048 ... 8192 points, evenly spaced sizes.  Everything is
seeded and made before the clock starts.  Both ways must return the same bits (asserted first).  For k = 2, 5 and 20: after
a warm-up the two ways alternate, in an order that reverses every repetition; a repetition is the wall-clock time between
two stream synchronisations.  Median and fastest of each go to stdout as one JSON line per k, and to --out when given.
Needs a GPU.

    python tools/time_knn_ragged.py [--reps 30] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIRS = 16
QUERIES = 5000
KS = (2, 5, 20)


def clustered(seed, n):
    rng = np.random.default_rng(seed)
    c = rng.random((5, 3)) - 0.5
    return (c[rng.integers(0, 5, n)] + 0.02 * rng.normal(size=(n, 3))).astype(np.float32)


def box_queries(seed, targets, n):
    rng = np.random.default_rng(seed)
    return rng.uniform(targets.min(axis=0), targets.max(axis=0), (n, 3)).astype(np.float32)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_knn_ragged: needs a GPU (a time taken elsewhere says nothing)")
    from genpc_amd.knn import knn_query, knn_query_ragged
    dev = torch.device("cuda", torch.cuda.current_device())
    sizes = [int(v) for v in np.linspace(2048, 8192, PAIRS)]
    host_t = [clustered(100 + j, m) for j, m in enumerate(sizes)]
    targets = [torch.from_numpy(t).to(dev) for t in host_t]
    queries = [torch.from_numpy(box_queries(200 + j, t, QUERIES)).to(dev) for j, t in enumerate(host_t)]
    packed_q = (torch.cat(queries).contiguous(), [QUERIES * j for j in range(PAIRS + 1)])
    packed_t = (torch.cat(targets).contiguous(), [0] + [int(v) for v in np.cumsum(sizes)])
    result = {"device": torch.cuda.get_device_name(dev), "pairs": PAIRS, "queries_per_pair": QUERIES, "target_sizes": sizes,
              "launches": {"ragged": 3, "loop": 3 * PAIRS}, "k": {}}
    for k in KS:
        fns = {"ragged": lambda: knn_query_ragged(packed_q, packed_t, k),
               "loop": lambda: [knn_query(q, t, k) for q, t in zip(queries, targets)]}
        got = {}
        for _ in range(args.warmup):
            for name, fn in fns.items():
                got[name] = fn()
        torch.cuda.synchronize()
        for j, ((d, i), (ld, li)) in enumerate(zip(got["ragged"][0], got["loop"])):
            assert torch.equal(d.view(torch.int32), ld.view(torch.int32)) and torch.equal(i, li), "k=%d pair %d: the two ways differ" % (k, j)
        times = {name: [] for name in fns}
        names = list(fns)
        for r in range(args.reps):
            for name in (names if r % 2 == 0 else names[::-1]):
                times[name].append(timed(fns[name]))
        row = {name: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "reps": len(v)} for name, v in times.items()}
        row["loop_over_ragged"] = row["loop"]["median_ms"] / row["ragged"]["median_ms"]
        result["k"][str(k)] = row
        print(json.dumps({"k": k, **row}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
