"""Times the fine xyz scale search over S scans two ways: the ragged forms (reg_xyz.scale_search_scores_ragged -- one library
call, two launches whatever S is, nothing written per candidate -- and reg_xyz.iterative_scale_searches end to end: one scores
call, one read-back, one ragged ICP over the winners) and the loop of the single-scan forms over the same scans
(genpc_scale_search_scores per scan: scaled copies of both clouds per candidate, nn_forward, cd_score_kernel; and
reg_xyz.iterative_scale_search per scan: two host stalls each) -- the only way before there was a ragged entry point, and a
code path this library leaves as it was.

The shape is reg()'s: S = 1, 4 and 16 scans of about 2500 source and 2700 target points (an ellipsoid's surface, seeded, the
sizes differ from scan to scan), 1000 candidates each (10 x 10 x 10 over 0.8 ... 1.2), cd_inv_weight 0.5.  Both ways must give
the same bits (asserted first).  After a warm-up the ways alternate, in an order that reverses every repetition.  The scores
calls are bracketed by HIP events on the stream; the searches, which read back, by the host clock between two synchronisations.

Median, 10th / 90th percentile and minimum of each go to profiles/scale_search_ragged_time.json.  Needs a GPU.

    python tools/scale_search_ragged_time.py [--reps 20] [--warmup 3] [--sizes 1,4,16] [--out profiles/scale_search_ragged_time.json]
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

NS, NT, STEPS, WEIGHT = 2500, 2700, 10, 0.5


def surface(seed, n):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (u * np.array([0.5, 0.3, 0.2]) + 0.05 * np.abs(u[:, :1])).astype(np.float32)


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "p10_ms": float(np.percentile(a, 10)), "p90_ms": float(np.percentile(a, 90)),
            "min_ms": float(a[0]), "reps": int(len(a))}


def timed_events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed_host(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(fns, reps, timed):
    """Every way once per repetition, the order reversed every other repetition."""
    t = {name: [] for name in fns}
    names = list(fns)
    for r in range(reps):
        for name in (names if r % 2 == 0 else names[::-1]):
            t[name].append(timed(fns[name]))
    return {name: stats(v) for name, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1,4,16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scale_search_ragged_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scale_search_ragged_time: needs a GPU (a time taken elsewhere says nothing)")
    from genpc_amd import _lib, reg_xyz
    dev = torch.device("cuda", torch.cuda.current_device())
    sizes = [int(v) for v in args.sizes.split(",")]
    xs = np.linspace(0.8, 1.2, STEPS)
    gz, gx, gy = np.meshgrid(xs, xs, xs, indexing="ij")
    cand = torch.from_numpy(np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1).astype(np.float32)).to(dev)
    k = cand.shape[0]
    src = [torch.from_numpy((surface(2000 + j, NS + 41 * (j % 5) - 80).astype(np.float64) * (0.9 + 0.01 * (j % 7))).astype(np.float32)).to(dev)
           for j in range(max(sizes))]
    tgt = [torch.from_numpy(surface(3000 + j, NT + 53 * (j % 4) - 70)).to(dev) for j in range(max(sizes))]
    ranges = [(0.8, 1.2)] * 3

    def scores_single(s, t, out):
        rc = _lib.on_device_of(s, _lib.lib.genpc_scale_search_scores, k, s.shape[0], _lib.ptr(s), t.shape[0], _lib.ptr(t), _lib.ptr(cand),
                               WEIGHT, _lib.ptr(out))
        assert rc == 1, _lib.last_error()

    result = {"device": torch.cuda.get_device_name(dev), "source_points": [int(s.shape[0]) for s in src], "target_points": [int(t.shape[0]) for t in tgt],
              "candidates_per_scan": int(k), "cd_inv_weight": WEIGHT, "launches": {"scores_ragged_call": 2},
              "clock": {"scores": "HIP events", "search": "host clock between synchronisations"}, "batches": {}}
    for s in sizes:
        S_, T_ = src[:s], tgt[:s]
        packed_s = (torch.cat(S_).contiguous(), np.cumsum([0] + [c.shape[0] for c in S_]).tolist())
        packed_t = (torch.cat(T_).contiguous(), np.cumsum([0] + [c.shape[0] for c in T_]).tolist())
        cands = [cand] * s
        loop_out = [torch.empty(k, device=dev) for _ in range(s)]
        score_fns = {"scores_ragged": lambda: reg_xyz.scale_search_scores_ragged(packed_s, packed_t, cands, cd_inv_weight=WEIGHT),
                     "scores_loop": lambda: [scores_single(a, b, o) for a, b, o in zip(S_, T_, loop_out)]}
        search_fns = {"search_ragged": lambda: reg_xyz.iterative_scale_searches(packed_s, packed_t, ranges, STEPS, cd_inv_weight=WEIGHT),
                      "search_loop": lambda: [reg_xyz.iterative_scale_search(a, b, ranges, STEPS, cd_inv_weight=WEIGHT) for a, b in zip(S_, T_)]}
        got = {}
        for _ in range(args.warmup):
            for name, fn in list(score_fns.items()) + list(search_fns.items()):
                got[name] = fn()
        torch.cuda.synchronize()
        for j in range(s):          # the same bits both ways, at the sizes that are timed
            assert torch.equal(got["scores_ragged"][j].view(torch.int32), loop_out[j].view(torch.int32)), "S=%d scan %d: other scores" % (s, j)
            a, b = got["search_ragged"][j], got["search_loop"][j]
            assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]), "S=%d scan %d: another search result" % (s, j)
        row = alternate(score_fns, args.reps, timed_events)
        row.update(alternate(search_fns, args.reps, timed_host))
        for name in row:
            row[name]["per_scan_ms"] = row[name]["median_ms"] / s
        row["scores_loop_over_ragged"] = row["scores_loop"]["median_ms"] / row["scores_ragged"]["median_ms"]
        row["search_loop_over_ragged"] = row["search_loop"]["median_ms"] / row["search_ragged"]["median_ms"]
        result["batches"]["S%d" % s] = row
        print("S=%d" % s, json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
