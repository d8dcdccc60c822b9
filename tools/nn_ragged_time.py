"""Times both Chamfer directions over a ragged batch two ways: genpc_nm_distance_ragged (one call per direction) and the
per-pair loop of genpc_nm_distance (B = 1 calls, the only way before there was a ragged entry point).

Two batches:
  * waymo59: the 59 Waymo car crops at their raw sizes against the complete car -- tests/golden/waymo_car59_4096.npz with every
    pad-repeated crop truncated to its count (a crop the fixture subsampled stays at 4096);
  * mix64: 64 synthetic pairs, sizes drawn from 100 .. 8192 (seeded).
Inputs are packed and outputs allocated before the clock starts, for both ways alike.  After a warm-up the two ways
alternate; each repetition is bracketed by HIP events on the stream.  Median, 10th / 90th percentile and minimum of
each, and the ratio of the medians, go to profiles/nn_ragged_time.json.  Needs a GPU.

--which dense times the ragged call's two searches against each other instead, search="grid" against search="dense" (all pairs,
csrc/nn_ragged_dense.hip), same protocol, into --dense-out.  Its batches are the ragged alignment loop's: 64
pairs of about 900 against 4 500 points, both directions --
  * pose64_aligned: the queries drawn on the targets' surface (every query has a near target: the grid search's best case);
  * pose64_turned: three of every four pairs with the queries turned by 90 / 180 / 270 degrees about the cloud's centre, as the
    loop's starts are (the grid search's lanes walk many cells);
  * pose64_far: the queries turned by 180 degrees and pushed four diameters away (no query has a near target);
  * big16_aligned: 16 pairs of 4 096 against 65 536 points, aligned -- larger targets, where all pairs cost the most.

    python tools/nn_ragged_time.py [--reps 40] [--warmup 5] [--which ragged|dense|both] [--out profiles/nn_ragged_time.json]
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


def surface(rng, n):
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (u * np.array([0.5, 0.3, 0.2])).astype(np.float32)


def dense_batches():
    """(queries, targets) pairs for the dense-against-grid comparison (the head of this file)."""
    rng = np.random.default_rng(45)
    out = {"pose64_aligned": [], "pose64_turned": [], "pose64_far": [], "big16_aligned": []}
    for j in range(64):
        n, m = 886 + 11 * (j % 6) - 17 * (j % 4), 4493 + 37 * (j % 7) - 53 * (j % 5)
        t = surface(rng, m)
        q = surface(rng, 4 * n)
        q = q[q[:, 2] > -0.05][:n]
        c = t.astype(np.float64).mean(0)
        th = np.radians(90.0 * (j % 4))
        R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
        out["pose64_aligned"].append((q, t))
        out["pose64_turned"].append(((c + (q - c) @ R.T).astype(np.float32), t))
        out["pose64_far"].append(((c - (q - c) * np.array([1, 1, -1]) + np.array([4.0, 0, 0])).astype(np.float32), t))
    for j in range(16):
        out["big16_aligned"].append((surface(rng, 4096), surface(rng, 65536)))
    return out


def time_dense(args, dev, _lib, chamfer_3D):
    result = {"device": torch.cuda.get_device_name(dev), "arith_mode": _lib.lib.genpc_get_arith(),
              "protocol": "one process; after %d warm-ups the grid and the dense call alternate, %d repetitions, each bracketed by HIP "
                          "events on the stream; q_to_t = the queries against the targets, t_to_q the converse" % (args.warmup, args.reps),
              "batches": {}}
    for name, pairs in dense_batches().items():
        PA = torch.from_numpy(np.concatenate([a for a, _ in pairs])).to(dev)
        PB = torch.from_numpy(np.concatenate([b for _, b in pairs])).to(dev)
        offa = [0] + list(np.cumsum([len(a) for a, _ in pairs]))
        offb = [0] + list(np.cumsum([len(b) for _, b in pairs]))
        outs = {s: [torch.empty(PA.shape[0], device=dev), torch.empty(PA.shape[0], device=dev, dtype=torch.int32),
                    torch.empty(PB.shape[0], device=dev), torch.empty(PB.shape[0], device=dev, dtype=torch.int32)] for s in ("grid", "dense")}

        def call(search, way):
            o = outs[search]
            if way == 0:
                assert chamfer_3D.nm_distance_ragged(PA, offa, PB, offb, o[0], o[1], search=search) == 1, _lib.last_error()
            else:
                assert chamfer_3D.nm_distance_ragged(PB, offb, PA, offa, o[2], o[3], search=search) == 1, _lib.last_error()

        def timed(search, way):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(search, way)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        for _ in range(args.warmup):
            for s in ("grid", "dense"):
                call(s, 0)
                call(s, 1)
        torch.cuda.synchronize()
        same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(outs["grid"], outs["dense"]))
        ts = {(s, w): [] for s in ("grid", "dense") for w in (0, 1)}
        for _ in range(args.reps):
            for key in ts:
                ts[key].append(timed(*key))
        entry = {"pairs": len(pairs), "queries": int(offa[-1]), "targets": int(offb[-1]), "same_bits": bool(same),
                 "pair_evaluations_per_direction": int(sum(len(a) * len(b) for a, b in pairs))}
        for s in ("grid", "dense"):
            entry[s] = {"q_to_t": stats(ts[(s, 0)]), "t_to_q": stats(ts[(s, 1)])}
        for w, way in ((0, "q_to_t"), (1, "t_to_q")):
            entry["grid_over_dense_" + way] = entry["grid"][way]["median_ms"] / entry["dense"][way]["median_ms"]
        result["batches"][name] = entry
        print(name, json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.dense_out)), exist_ok=True)
    with open(args.dense_out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.dense_out}))


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "p10_ms": float(np.percentile(a, 10)), "p90_ms": float(np.percentile(a, 90)),
            "min_ms": float(a[0]), "reps": int(len(a))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nn_ragged_time.json"))
    ap.add_argument("--which", default="ragged", choices=("ragged", "dense", "both"))
    ap.add_argument("--dense-out", default=os.path.join(ROOT, "profiles", "nn_ragged_dense_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nn_ragged_time: needs a GPU (a time taken elsewhere says nothing)")
    from genpc_amd import _lib, chamfer_3D
    dev = torch.device("cuda", torch.cuda.current_device())
    if args.which in ("dense", "both"):
        time_dense(args, dev, _lib, chamfer_3D)
    if args.which == "dense":
        return
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
