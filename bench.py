#!/usr/bin/env python3
"""bench.py -- headline benchmark of the GenPC geometric hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the K steps and prints the headline line (contract fields,
`ranks_seen`, `config`); nothing else runs in it.  `--full` adds everything else listed below: the
per-step spread, the roofline figures (a pass of their own through the filter kernel's events), the
oracle check of the timed step's output, `extra` and `cpu_baseline` (`--no-extra` / `--no-cpu-baseline`
drop those two).  `--dump-outputs DIR` writes what the last timed step computed, the arrays a caller of
`chamfer_3DDist.forward` receives (dist1, dist2, idx1, idx2; the gathered scan table for --workload), as
DIR/<name>.npy (see dump_outputs); the inputs are seeded, so two builds compare output for output.

Workload (BASELINE.json metric "Chamfer Gpair-dist/sec", SURVEY.md section 8d headline):
one STEP = one `chamfer_3DDist.forward` (both directions, i.e. 2*N*M pair
evaluations) on one synthetic pair of clouds, B=1, N=M=16384, fp32, through the C
ABI of libgenpc_hip.so, inputs resident in HBM.  `rng=default_rng(20250101)`,
`A,B = rng.random((1,N,3),float32)-0.5`.  With --gpus N every rank runs the same
per-rank workload on its own pair (independent scans shard with no data-path
collective): weak scaling, value = total pair-dist/s over all ranks.

`python bench.py --gpus N` without a torchrun environment starts the torchrun form itself as a
child process (before anything touches a GPU) and exits with its code; a run whose realised
world size differs from --gpus exits non-zero.  `--workload c3|c4|c5` times the scan-sharded
workloads of BASELINE configs 3 / 4 / 5 instead of the pair benchmark (13 bundled scans' CD + EMD metric; 59 Waymo
CAR crops registered against a complete car; 64 synthetic scans registered + scored -- strong scaling:
the scans are dealt round-robin over the ranks, metric completed scans/s, every rank's own time in `per_rank`).

One JSON line on stdout (rank 0).  Besides the contract fields, with --full:
  roofline      the dominant kernel (nn_f16_kernel, the MFMA filter that evaluates every
                pair) against the dense f16 MFMA roofline, 2500 TFLOP/s: one K = 16
                product per pair = 32 flop/pair of matrix work;
                duration = HIP events around that kernel alone (genpc_nn_profile).
                "step_frac_fp32_valu" prices the WHOLE step at SURVEY 8d's 8 flop per pair
                (3 sub, 3 mul, 2 add) against the 157.3 TFLOP/s fp32 vector peak, the roofline a
                brute-force fp32 kernel would be held to (an equivalent rate: the pairs are
                evaluated on the f16 matrix pipe).  "traffic" = HBM bytes per launch from THIS
                round's committed PMC profile (profiles/r04_chamfer_B1_16384.json), else null.
  roofline_hbm  the same launch against the 8 TB/s HBM roofline (algorithmic bytes
                20*(N+M) per call); north_star asks for it; it is << 1 % by nature.
  cpu_baseline  the CPU oracle (a port: the reference has no CPU path) timed on the
                host cores on a bounded sample of the same workload.
  extra         secondary measurements (EMD, backward, metric scans/s).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_PTS = 16384
SEED = 20250101
PEAK_FP32_TFLOPS = 157.3
PEAK_F16_MFMA_TFLOPS = 2500.0
MFMA_FLOP_PER_PAIR = 32      # K = 16 multiply-adds per pair on v_mfma_f32_32x32x16_f16
PEAK_HBM_GBS = 8000.0
FLOP_PER_PAIR = 8


def make_pair(n, seed, device):
    rng = np.random.default_rng(seed)
    a = rng.random((1, n, 3), dtype=np.float32) - np.float32(0.5)
    b = rng.random((1, n, 3), dtype=np.float32) - np.float32(0.5)
    return torch.from_numpy(a).to(device), torch.from_numpy(b).to(device), a, b


def time_events(fn, reps, stream):
    """Average duration (ms) of `fn` over `reps` calls, HIP events on `stream`."""
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


DUMP_LIMIT_BYTES = 64 * 10 ** 6


def dump_outputs(where, arrays, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: every array as where/<name>.npy, float32 / float16 as float32, everything else (the int32
    indices included, exactly) as float64.  Above `limit` bytes in all, every array keeps the same fixed, seeded
    sample of its flat positions, in order, so that two runs or two builds still compare element for element."""
    os.makedirs(where, exist_ok=True)
    out = {}
    for name, a in arrays.items():
        a = np.asarray(a)
        out[name] = a.astype(np.float32 if a.dtype in (np.float32, np.float16) else np.float64)
    total = sum(a.nbytes for a in out.values())
    if total > limit:
        budget = limit - 4096 * len(out)          # (room for the .npy headers)
        for name, a in out.items():
            keep = a.size * budget // total
            out[name] = a.reshape(-1)[np.sort(np.random.default_rng(SEED).choice(a.size, keep, replace=False))]
    for name, a in out.items():
        np.save(os.path.join(where, name + ".npy"), a)


ROUND_TAG = "r06"          # the profiles/ tag this bench's PMC-derived numbers must come from


def pmc_traffic(n, kernel_prefix="nn_f16_kernel"):
    """HBM bytes per launch of the dominant kernel from THIS round's committed rocprofv3 PMC passes
    (profiles/<ROUND_TAG>_chamfer_B1_<n>.json, written by tools/collect_profiles.sh +
    tools/summarize_profiles.py: FETCH_SIZE and WRITE_SIZE collected in separate runs, FETCH_SIZE
    doubled per MI355X_MICROARCH.md section HBM).  Returns (bytes or None, source): a missing or
    older-tagged profile is reported on stderr and yields None -- never a stale number."""
    f = os.path.join(ROOT, "profiles", "%s_chamfer_B1_%d.json" % (ROUND_TAG, n))
    try:
        d = json.load(open(f))
    except Exception as e:
        print("bench.py: roofline.traffic unavailable: %s (%s); run tools/collect_profiles.sh %s on the GPU box"
              % (os.path.relpath(f, ROOT), type(e).__name__, ROUND_TAG), file=sys.stderr)
        return None, None
    if d.get("tag") != ROUND_TAG:
        print("bench.py: %s carries tag %r, not %r: refusing a stale traffic figure" % (f, d.get("tag"), ROUND_TAG), file=sys.stderr)
        return None, None
    for name, k in d.get("kernels", {}).items():
        if name.startswith(kernel_prefix) and k.get("hbm_bytes_per_launch") is not None:
            return k["hbm_bytes_per_launch"], os.path.relpath(f, ROOT)
    print("bench.py: no %s* kernel with PMC counters in %s" % (kernel_prefix, f), file=sys.stderr)
    return None, None


def extras(A, B, n, dev, stream):
    """Secondary measurements (not the headline): other sizes, backward, EMD, the
    streaming kernels against the HBM roofline, and scans/s of the alignment loop."""
    from genpc_amd import chamfer_3D
    from genpc_amd.loss_functions import chamfer_3DDist, emdModule
    from genpc_amd.DepthPrompting import DepthPrompting, create_cameras
    from genpc_amd.optim_registration.diff_obj_pose import object_pose_optimization
    from genpc_amd.utils.loss_util import Completionloss
    from types import SimpleNamespace
    extra = {}
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED)          # every synthetic input of the extras is reproducible
    cd = chamfer_3DDist()
    Ag = A.clone().requires_grad_(True)
    Bg = B.clone().requires_grad_(True)

    def fb():
        Ag.grad = None
        Bg.grad = None
        d1, d2, _, _ = cd(Ag, Bg)
        (torch.sqrt(d1).mean() + torch.sqrt(d2).mean()).backward()
    fb()
    extra["chamfer_fwd_bwd_autograd_ms"] = round(time_events(fb, 20, stream), 4)
    for nn in (2048, 4096, 8192, 32768):
        P, Q, _, _ = make_pair(nn, SEED, dev)
        d1 = torch.empty(1, nn, device=dev)
        d2 = torch.empty(1, nn, device=dev)
        i1 = torch.empty(1, nn, device=dev, dtype=torch.int32)
        i2 = torch.empty(1, nn, device=dev, dtype=torch.int32)
        f = lambda: chamfer_3D.forward(P, Q, d1, d2, i1, i2)  # noqa: E731
        f()
        t = time_events(f, 50, stream)
        extra["chamfer_fwd_B1_n%d_gpair_s" % nn] = round(2.0 * nn * nn / (t * 1e-3) / 1e9, 2)
    # BASELINE config 3 shape: 13 scans x 16384 in one batched call
    P13 = torch.rand(13, n, 3, device=dev, generator=gen) - 0.5
    Q13 = torch.rand(13, n, 3, device=dev, generator=gen) - 0.5
    o = [torch.empty(13, n, device=dev), torch.empty(13, n, device=dev),
         torch.empty(13, n, device=dev, dtype=torch.int32), torch.empty(13, n, device=dev, dtype=torch.int32)]
    f = lambda: chamfer_3D.forward(P13, Q13, o[0], o[1], o[2], o[3])  # noqa: E731
    f()
    t = time_events(f, 10, stream)
    g13 = 13 * 2.0 * n * n / (t * 1e-3) / 1e9
    extra["chamfer_fwd_B13_n%d_gpair_s" % n] = round(g13, 2)
    # How often the f16 filter's proof fails (the query is re-done exhaustively; genpc_nn_stats): the bench input, the 13
    # bundled scans, the Waymo crops (13 of 59 pad-repeated) against the complete car, and SURVEY 8d's C5 scans (partial
    # clouds resampled with replacement: a third of the points are exact triplicates or more).  "first": a call that
    # finds the duplicate pre-pass off (csrc/nn_dedupe.hip); "steady": the following calls, switched by the policy
    import ctypes
    gold = os.path.join(ROOT, "tests", "golden")
    share = {}

    def redo_share(name, P, Q):
        P, Q = P.contiguous(), Q.contiguous()
        o = [torch.empty(P.shape[0], P.shape[1], device=dev), torch.empty(Q.shape[0], Q.shape[1], device=dev),
             torch.empty(P.shape[0], P.shape[1], device=dev, dtype=torch.int32), torch.empty(Q.shape[0], Q.shape[1], device=dev, dtype=torch.int32)]
        buf = (ctypes.c_ulonglong * 3)()
        clean = torch.rand(1, 4096, 3, device=dev, generator=gen)
        oc = [torch.empty(1, 4096, device=dev), torch.empty(1, 4096, device=dev), torch.empty(1, 4096, device=dev, dtype=torch.int32),
              torch.empty(1, 4096, device=dev, dtype=torch.int32)]
        for _ in range(3):                      # clean calls: whatever came before, the policy's switch is off again
            chamfer_3D.forward(clean, clean.flip(1).contiguous(), oc[0], oc[1], oc[2], oc[3])
            torch.cuda.synchronize()
        _lib.lib.genpc_nn_tune(-1, 512)
        row = []
        try:
            for _ in range(3):
                _lib.lib.genpc_nn_stats(ctypes.cast(buf, ctypes.c_void_p), 1, None)
                chamfer_3D.forward(P, Q, o[0], o[1], o[2], o[3])
                torch.cuda.synchronize()
                _lib.lib.genpc_nn_stats(ctypes.cast(buf, ctypes.c_void_p), 1, None)
                row.append(round(float(buf[1]) / max(1.0, float(buf[0])), 6))
        finally:
            _lib.lib.genpc_nn_tune(-1, 0)
        share[name] = {"first": row[0], "steady": row[-1]}

    from genpc_amd import _lib
    redo_share("bench_input_1x%d" % n, A, B)
    z13 = np.load(os.path.join(gold, "scans13_fps16384.npz"))

    def c2_probe(where):
        # diagnosis (GENPC_BENCH_C2_PROBES=1): the completed-scan line timed at several points of this function
        sel = os.environ.get("GENPC_BENCH_C2_PROBES", "0")
        if sel == "0" or (sel != "1" and sel != where):
            return
        from genpc_amd import pipeline as _plp
        st_ = c2_probe.__dict__
        if "cfg" not in st_:
            g0 = z13["gt"][0]
            cc0 = (g0.max(0) + g0.min(0)) / 2
            th0 = np.deg2rad(9.0)
            ax0 = np.array([0.2, 1.0, 0.1]) / np.linalg.norm([0.2, 1.0, 0.1])
            K0 = np.array([[0, -ax0[2], ax0[1]], [ax0[2], 0, -ax0[0]], [-ax0[1], ax0[0], 0]])
            R0 = np.eye(3) + np.sin(th0) * K0 + (1 - np.cos(th0)) * K0 @ K0
            st_["gen"] = torch.from_numpy((((g0 - cc0) / (g0.max(0) - g0.min(0)).max()).astype(np.float64) @ R0.T).astype(np.float32)).to(dev)
            st_["part"] = torch.from_numpy(z13["partial"][0][:8192].copy()).to(dev)
            st_["gt"] = torch.from_numpy(g0.copy()).to(dev)
            st_["img"] = torch.rand(3, 1024, 1024, device=dev)
            st_["cfg"] = _plp.default_cfg(str(dev), view_num=1024)
            st_["dp"] = DepthPrompting(st_["cfg"])
        a_ = (st_["part"], st_["gen"], st_["img"], st_["gt"])
        _plp.complete_scan(*a_, cfg=st_["cfg"], dp=st_["dp"])
        torch.cuda.synchronize()
        t0_ = time.perf_counter()
        for _ in range(4):
            _plp.complete_scan(*a_, cfg=st_["cfg"], dp=st_["dp"])
        torch.cuda.synchronize()
        print("[c2 probe] %-28s %.2f scans/s" % (where, 4.0 / (time.perf_counter() - t0_)), file=sys.stderr, flush=True)
    c2_probe("start")
    redo_share("bundled_scans_13x16384", torch.from_numpy(z13["partial"]).to(dev), torch.from_numpy(z13["gt"]).to(dev))
    zw = np.load(os.path.join(gold, "waymo_car59_4096.npz"))
    redo_share("waymo_crops_59x4096_vs_complete_car", torch.from_numpy(np.repeat(zw["complete"][None], 59, 0)).to(dev),
               torch.from_numpy(zw["crops"]).to(dev))
    sc5 = [synth_scan(k, 32768) for k in range(8)]
    redo_share("c5_scans_8x32768_complete_vs_resampled_partial", torch.from_numpy(np.stack([x[0] for x in sc5])).to(dev),
               torch.from_numpy(np.stack([x[1] for x in sc5])).to(dev))
    share["how"] = "queries re-done by the exhaustive pass / queries, one chamfer forward each (genpc_nn_stats, hook 512)"
    extra["nn_exhaustive_share"] = share
    em = emdModule()
    X = A + 0.5
    Y = B + 0.5
    em(X, Y, 0.005, 50)
    t_emd = time_events(lambda: em(X, Y, 0.005, 50), 5, stream)
    extra["emd_fwd_n%d_eps0.005_it50_ms" % n] = round(t_emd, 4)
    # roofline-shaped entry for the auction: algorithmic pairs = sum over rounds of (bidders x objects);
    # bidders of round k - 1 = the list length a k-round call leaves in its ping-pong count buffers
    from genpc_amd import emd as emd_abi
    from genpc_amd.loss_functions.emd.emd_module import alloc_state
    pairs = 0.0
    prev_impl = _lib.lib.genpc_emd_tune(1, -1)      # (the bidder counts live in the launch-per-round path's list buffers)
    try:
        for k in range(1, 51):
            st = alloc_state(1, n, n, dev)
            emd_abi.forward(X, Y, st["dist"], st["assignment"], st["price"], st["assignment_inv"], st["bid"],
                            st["bid_increments"], st["max_increments"], st["unass_idx"], st["unass_cnt"], st["unass_cnt_sum"],
                            st["cnt_tmp"], st["max_idx"], 0.005, k)
            pairs += float((st["unass_cnt"] if (k - 1) % 2 == 0 else st["cnt_tmp"])[0].item()) * n
    finally:
        _lib.lib.genpc_emd_tune(prev_impl, -1)
    extra["emd_fwd_n%d_roofline" % n] = {
        "bound": "valu-fp32", "unit": "TFLOP/s", "algorithmic_pairs_per_call": pairs, "pairs_over_n2": round(pairs / n / n, 3),
        "flop_per_pair": FLOP_PER_PAIR, "ms_per_call": round(t_emd, 4),
        "achieved": round(FLOP_PER_PAIR * pairs / (t_emd * 1e-3) / 1e12, 3), "peak": PEAK_FP32_TFLOPS,
        "frac": round(FLOP_PER_PAIR * pairs / (t_emd * 1e-3) / 1e12 / PEAK_FP32_TFLOPS, 4),
        "note": "all 50 rounds in one launch whose threads own the points (csrc/emd_auction.hip), latency-bound at B=1: ~12 dependent global round trips and two barriers per round; algorithmic pairs = bidders x ALL objects per round (the culled bid tests ~70 of 16384 per bidder)"}
    # the same call through the launch-per-round path (round 4's default), for continuity
    prev_impl = _lib.lib.genpc_emd_tune(1, -1)
    try:
        em(X, Y, 0.005, 50)
        extra["emd_fwd_n%d_launch_per_round_ms" % n] = round(time_events(lambda: em(X, Y, 0.005, 50), 5, stream), 4)
    finally:
        _lib.lib.genpc_emd_tune(prev_impl, -1)
    # BASELINE config 3's EMD half: the 13 bundled scans against their ground truth in one call (most points keep
    # bidding for all 50 rounds there -- the regime the bid's culling was built for), and 13 uniform pairs for scale
    P13s, G13s = torch.from_numpy(z13["partial"]).to(dev), torch.from_numpy(z13["gt"]).to(dev)
    em(P13s, G13s, 0.005, 50)
    torch.cuda.synchronize()          # (the first call's bidder count decides the path of the next ones: it must have arrived)
    em(P13s, G13s, 0.005, 50)
    torch.cuda.synchronize()
    extra["emd_fwd_13_bundled_scans_n%d_ms" % n] = round(time_events(lambda: em(P13s, G13s, 0.005, 50), 3, stream), 3)
    U13a, U13b = P13 + 0.5, Q13 + 0.5
    em(U13a, U13b, 0.005, 50)
    torch.cuda.synchronize()
    em(U13a, U13b, 0.005, 50)
    torch.cuda.synchronize()
    extra["emd_fwd_B13_uniform_n%d_ms" % n] = round(time_events(lambda: em(U13a, U13b, 0.005, 50), 3, stream), 3)
    X2 = X[:, :2048].contiguous()
    Y2 = Y[:, :2048].contiguous()
    em(X2, Y2, 0.005, 50)
    extra["emd_fwd_n2048_eps0.005_it50_ms"] = round(time_events(lambda: em(X2, Y2, 0.005, 50), 5, stream), 4)
    # metric pass of one completed scan (main.metric: CD-L1 + EMD at 16384 points)
    cl1, cle = Completionloss("cd_l1"), Completionloss("emd")

    def metric():
        cl1.get_loss(X, Y)
        cle.get_loss(X, Y)
    metric()
    extra["metric_cd_emd_n%d_scans_per_s" % n] = round(1e3 / time_events(metric, 5, stream), 2)
    # alignment loop (diff_obj_pose, full objective: mask + 3 cd + ortho): 8192-point partial vs
    # 16384-point complete, 4 starts x 201 Adam steps, then the metric above = one "completed scan"
    C16 = A[0]
    P8 = (B[0, :8192] * 0.9).contiguous()
    object_pose_optimization(C16, P8, radius=0.02, lr=0.01, iters=200, render_size=224)

    def scan():
        object_pose_optimization(C16, P8, radius=0.02, lr=0.01, iters=200, render_size=224)
        metric()
    t0 = time.perf_counter()
    for _ in range(3):
        scan()
    torch.cuda.synchronize()
    extra["registration_8k_vs_16k_4x201_plus_metric_scans_per_s"] = round(3.0 / (time.perf_counter() - t0), 3)
    # ... six such single-scan registrations in flight side by side (independent scans; pipeline.run_in_lanes)
    from genpc_amd import pipeline as _pl1
    _pl1.run_in_lanes(lambda li, _: scan(), range(6), 6, dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _pl1.run_in_lanes(lambda li, _: scan(), range(18), 6, dev)
    torch.cuda.synchronize()
    extra["registration_8k_vs_16k_6_scans_in_flight_scans_per_s"] = round(18.0 / (time.perf_counter() - t0), 3)
    # the same, 8 scans in lock-step (one batched NN launch per Adam step) + batched metric
    c2_probe("after emd + registration lanes")
    C8 = (torch.rand(8, n, 3, device=dev, generator=gen) - 0.5)
    P8b = (C8[:, :8192] * 0.9).contiguous()
    X8, Y8 = C8 + 0.5, (C8.flip(0) + 0.5).contiguous()
    from genpc_amd.metric import evaluate_scans
    object_pose_optimization(C8, P8b, radius=0.02, lr=0.01, iters=200, render_size=224)
    evaluate_scans(X8, Y8)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    object_pose_optimization(C8, P8b, radius=0.02, lr=0.01, iters=200, render_size=224)
    evaluate_scans(X8, Y8)
    torch.cuda.synchronize()
    extra["registration_batch8_8k_vs_16k_4x201_plus_metric_scans_per_s"] = round(8.0 / (time.perf_counter() - t0), 3)
    # ... and three such groups in flight side by side (pipeline.run_in_lanes: a host thread and a stream per group)
    from genpc_amd import pipeline as _pl

    def group8(li, _):
        object_pose_optimization(C8, P8b, radius=0.02, lr=0.01, iters=200, render_size=224)
        return evaluate_scans(X8, Y8)
    _pl.run_in_lanes(group8, range(3), 3, dev)
    torch.cuda.synchronize()
    # (twelve groups, two timings: one timing of six groups read 57 once where every other run of the round read 80-86)
    rates = []
    for _ in range(2):
        t0 = time.perf_counter()
        _pl.run_in_lanes(group8, range(6), 3, dev)
        torch.cuda.synchronize()
        rates.append(48.0 / (time.perf_counter() - t0))
    extra["registration_batch8_3_groups_in_flight_scans_per_s"] = round(sum(rates) / len(rates), 3)
    extra["registration_batch8_3_groups_in_flight_two_timings"] = [round(r, 1) for r in rates]
    # the same without the silhouette term (round 1's objective), for continuity
    object_pose_optimization(C8, P8b, lr=0.01, iters=200, cd_only=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    object_pose_optimization(C8, P8b, lr=0.01, iters=200, cd_only=True)
    evaluate_scans(X8, Y8)
    torch.cuda.synchronize()
    extra["registration_batch8_cd_only_scans_per_s"] = round(8.0 / (time.perf_counter() - t0), 3)
    # a17: the 1000-candidate anisotropic scale search of reg() (voxel-0.03 clouds are a few
    # thousand points) -- one batched NN launch + one ICP -- and an 11-candidate coarse sweep
    c2_probe("after batch8 groups")
    from genpc_amd import reg_xyz
    src3k = (A[0, :3000] * 0.9).contiguous()
    tgt3k = A[0, :4000].contiguous()
    reg_xyz.iterative_scale_search(src3k, tgt3k, [(0.8, 1.2)] * 3, 10, cd_inv_weight=0.5)
    t0 = time.perf_counter()
    for _ in range(3):
        reg_xyz.iterative_scale_search(src3k, tgt3k, [(0.8, 1.2)] * 3, 10, cd_inv_weight=0.5)
    torch.cuda.synchronize()
    extra["scale_search_1000cand_3000x4000_ms"] = round((time.perf_counter() - t0) / 3 * 1e3, 3)
    reg_xyz.coarse_scale_sweep(src3k, tgt3k, cd_inv_weight=0.5)
    t0 = time.perf_counter()
    for _ in range(3):
        reg_xyz.coarse_scale_sweep(src3k, tgt3k, cd_inv_weight=0.5)
    torch.cuda.synchronize()
    extra["coarse_sweep_11scales_2icp_each_ms"] = round((time.perf_counter() - t0) / 3 * 1e3, 3)
    # f2: deterministic FPS, 4 clouds x 165546 -> 16384 (the metric's subsampling, main.py:21-24)
    from genpc_amd.fps import fps_sampling
    big = torch.rand(4, 165546, 3, device=dev, generator=gen)
    fps_sampling(big, 64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fps_sampling(big, 16384)
    torch.cuda.synchronize()
    t_fps = time.perf_counter() - t0
    extra["fps_4x165546_to_16384_ms"] = round(t_fps * 1e3, 2)
    # roofline-shaped: the O(n k) work of FPS is one distance update per (point, sample): 8 algorithmic flop (3 sub,
    # 3 mul / fma, 1 min ... priced like a pair of SURVEY 8d) against the fp32 vector peak.  The path is NOT bound by
    # that: the k samples are sequential, and what a step costs is the dependency chain that picks the next sample
    # (csrc/fps.hip: one inter-workgroup exchange yields ~45 samples, replayed by one wave at ~900 cycles each)
    upd = 4.0 * 165546 * 16384
    extra["fps_4x165546_to_16384_roofline"] = {
        "bound": "valu-fp32", "unit": "TFLOP/s", "flop_per_point_update": 8, "point_updates": upd,
        "achieved": round(8 * upd / t_fps / 1e12, 2), "peak": PEAK_FP32_TFLOPS, "frac": round(8 * upd / t_fps / 1e12 / PEAK_FP32_TFLOPS, 4),
        "us_per_sequential_step": round(t_fps * 1e6 / 16384, 3), "clouds_side_by_side": 4,
        "note": "latency-bound by construction (sequential argmax chain); round 2: 2.8 us per step"}
    # ... and the two samplings of a completed scan's tail (pipeline.complete_scan): the fused cloud 24576 -> 20000 and the
    # metric's 20000 -> 16384, on a bundled scan's surface -- the one-workgroup pruned sampling of csrc/fps_grid.hip
    try:
        zf = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "golden", "scans13_fps16384.npz"))
        surf = torch.from_numpy(np.concatenate([zf["partial"][0][:8192], zf["gt"][0]]).astype(np.float32)).to(dev)
        for key, cloud, k in (("fps_scan_24576_to_20000_ms", surf, 20000), ("fps_scan_20000_to_16384_ms", surf[:20000].contiguous(), 16384)):
            fps_sampling(cloud, 64)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                fps_sampling(cloud, k)
            torch.cuda.synchronize()
            extra[key] = round((time.perf_counter() - t0) / 3 * 1e3, 3)
    except Exception as e:
        extra["fps_scan_error"] = "%s: %s" % (type(e).__name__, e)
    # HBM-bound streaming kernel: getUvs for the reference's 1024 cameras x 71372 points
    cfg = SimpleNamespace(device=str(dev), fovy=49.1, res=256, padding=0.15, rescale=True, point_size=1,
                          mask_pixel_rate=3, view_num=1024, distance=1.6)
    dp = DepthPrompting(cfg)
    pts = (torch.rand(71372, 3, device=dev, generator=gen) - 0.5) * 0.8
    for _ in range(100):        # the clocks settle over tens of milliseconds (5-call averages read 245-275 us, 300-call ones 221)
        dp.getUvs(dp.cameras, pts, want_transformed=False)
    t = time_events(lambda: dp.getUvs(dp.cameras, pts, want_transformed=False), 100, stream)
    # algorithmic bytes: the cloud is read once (12 B per POINT, not per (camera, point)), uv + depth are written
    # per (camera, point): 12 N + 12 C N
    alg = 12 * 71372 + 1024 * 71372 * 12
    extra["get_uvs_1024x71372_roofline"] = {"bound": "hbm", "achieved": round(alg / (t * 1e-3) / 1e9, 1), "peak": PEAK_HBM_GBS,
                                            "unit": "GB/s", "frac": round(alg / (t * 1e-3) / 8e12, 4),
                                            "frac_of_6.29TBs_achievable": round(alg / (t * 1e-3) / 6.29e12, 4),
                                            "ms_per_call": round(t, 4), "algorithmic_bytes": alg,
                                            "bytes_model": "12 N read + 12 C N written (uv 8 + depth 4)"}
    # the other HBM-bound rows of SURVEY 8(a) -- a3 chamfer backward, a8 CalcDist, a10 EMD backward, the pose point map, a14
    # paintPixels, a15 colour gather -- at 64 x 32768 points (every 8(a) row gets a driver-visible frac)
    c2_probe("after fps + uvs")
    from genpc_amd import streaming_bench
    extra["streaming_rooflines_64x32768"] = streaming_bench.rooflines(dev, stream, reps=20)
    # f3: hidden-point removal (Katz' operator, exact) at viewpoint_select's shape -- the reference's 1024
    # viewpoints x 10000 FPS-ordered points, removal_radius 10000 -- and at getDepth's (2 viewpoints x the
    # whole scan); next to it qhull (what open3d calls) on one host core for ONE viewpoint
    c2_probe("after streaming")
    cfgh = SimpleNamespace(device=str(dev), fovy=49.1, res=256, cam_res=256, padding=0.15, rescale=True, point_size=1,
                           mask_pixel_rate=3, view_num=1024, distance=1.6, downsample_num=10000, removal_radius=10000)
    dph = DepthPrompting(cfgh)
    rngh = np.random.default_rng(5)
    vh = rngh.normal(size=(165546, 3))
    vh /= np.linalg.norm(vh, axis=1, keepdims=True)
    scan = torch.from_numpy((vh * (0.3 + 0.2 * np.abs(np.sin(3 * vh[:, :1])))).astype(np.float32)).to(dev)
    sub = scan[fps_sampling(scan, 10000).long()].contiguous()
    for name, p_, e_ in (("hpr_1024x10000", sub, dph.viewpoints), ("hpr_2x165546", scan, dph.viewpoints[:2])):
        dph.hidden_point_removal(p_, e_, 10000.0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, cnt_h, second_h = dph.hidden_point_removal(p_, e_, 10000.0, want_second=True)
        torch.cuda.synchronize()
        t_h = time.perf_counter() - t0
        extra[name + "_R10000_ms"] = round(t_h * 1e3, 2)
        extra[name + "_visible_fraction"] = round(float(cnt_h.float().mean()) / p_.shape[0], 4)
        # roofline-shaped: the brute-force operator tests every (view, point, other point) triple once (one fp64
        # dot product + compare = 6 flop); the culled kernels are priced against that algorithmic count
        v_, n_ = (len(e_), p_.shape[0])
        tests = float(v_) * n_ * (n_ - 1)
        extra[name + "_roofline"] = {"bound": "valu-fp64", "unit": "Gtest/s (algorithmic candidate tests: views x n x (n-1))",
                                     "achieved": round(tests / t_h / 1e9, 1), "peak": round(78.6e12 / 6 / 1e9, 1),
                                     "frac": round(tests / t_h / (78.6e12 / 6), 4),
                                     "note": "peak = 78.6 TFLOP/s fp64 vector / 6 flop per test; culling skips most tests, "
                                             "so frac is an equivalent rate, not a utilisation"}
    # viewpoint_select's own pass: views that can no longer see the most points are dropped after the first polygon kernel
    dph.hidden_point_removal(sub, dph.viewpoints, 10000.0, best_only=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, cnt_b, _ = dph.hidden_point_removal(sub, dph.viewpoints, 10000.0, best_only=True)
    torch.cuda.synchronize()
    extra["hpr_1024x10000_best_view_only_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    _, cnt_f, _ = dph.hidden_point_removal(sub, dph.viewpoints, 10000.0)
    extra["hpr_best_view_equals_full_pass"] = bool(int(torch.argmax(cnt_b)) == int(torch.argmax(cnt_f)))
    from oracle import hpr as ohpr
    t0 = time.perf_counter()
    ref_cnt = ohpr.visible_counts(sub.cpu().numpy(), np.asarray(dph.viewpoints)[:4], 10000.0)
    extra["hpr_cpu_qhull_ms_per_viewpoint_10000pts_1core"] = round((time.perf_counter() - t0) / 4 * 1e3, 2)
    _, cnt4, _ = dph.hidden_point_removal(sub, dph.viewpoints[:4], 10000.0)
    extra["hpr_counts_equal_qhull"] = bool((cnt4.cpu().numpy() == ref_cnt).all())
    # BASELINE config 2: the chained geometric stages of one completed scan (8192-point partial scan,
    # 16384-point generated shape): DepthPrompting -> colorPoint -> reg -> fuse -> metric.  Inputs as SURVEY 8g
    # prescribes: a bundled scan (tests/golden/scans13_fps16384.npz, scan 01184) and its ground-truth cloud under a
    # similarity transform as the "generated" shape (its own frame and scale, what the image-to-3D model returns).
    # (Rounds 1-3 timed this line on uniform VOLUME clouds -- almost every point interior: the worst case of the
    # hidden-point removal and not what a scan looks like; that figure is kept below as ..._uniform_volume.)
    c2_probe("after hpr")
    from genpc_amd import pipeline
    cfg2 = pipeline.default_cfg(str(dev), view_num=1024)
    dp2 = DepthPrompting(cfg2)
    gt0 = z13["gt"][0]
    cc = (gt0.max(0) + gt0.min(0)) / 2
    th = np.deg2rad(9.0)
    ax = np.array([0.2, 1.0, 0.1]) / np.linalg.norm([0.2, 1.0, 0.1])
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    Rg = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    gen_np = (((gt0 - cc) / (gt0.max(0) - gt0.min(0)).max()).astype(np.float64) @ Rg.T).astype(np.float32)
    part_s = torch.from_numpy(z13["partial"][0][:8192].copy()).to(dev)
    gen_s, gt_s = torch.from_numpy(gen_np).to(dev), torch.from_numpy(gt0.copy()).to(dev)
    img = torch.rand(3, 1024, 1024, device=dev, generator=gen)
    for name, a_part, a_gen, a_gt in (("c2_pipeline_8192_scans_per_s", part_s, gen_s, gt_s),
                                      ("c2_pipeline_8192_uniform_volume_scans_per_s", (B[0, :8192] * 0.9 + 0.01).contiguous(), A[0], A[0])):
        # (three untimed scans, eight timed: the line before this one ends in seconds of host-side qhull with the device idle, and
        #  the first scans behind an idle period read 26.6 where the same line behind a busy one reads 28.9 -- GENPC_BENCH_C2_PROBES)
        for _ in range(3):
            pipeline.complete_scan(a_part, a_gen, img, a_gt, cfg=cfg2, dp=dp2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(8):
            pipeline.complete_scan(a_part, a_gen, img, a_gt, cfg=cfg2, dp=dp2)
        torch.cuda.synchronize()
        extra[name] = round(8.0 / (time.perf_counter() - t0), 3)
    # completed scans per second is a throughput: six independent scans in flight on the one GPU (pipeline.complete_scans:
    # a host thread and a stream pair per lane; every scan's products are the bits of a call of its own)
    lanes_c2 = 6
    jobs_c2 = [(part_s, gen_s, img, gt_s)] * (8 * lanes_c2)      # (48 scans: 24 read 34-35 scans/s where long runs of the same lanes read 39-43)
    dps_c2 = [DepthPrompting(cfg2) for _ in range(lanes_c2)]
    pipeline.complete_scans(jobs_c2[:lanes_c2], lanes=lanes_c2, cfg=cfg2, dps=dps_c2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pipeline.complete_scans(jobs_c2, lanes=lanes_c2, cfg=cfg2, dps=dps_c2)
    torch.cuda.synchronize()
    extra["c2_pipeline_8192_scans_in_flight"] = lanes_c2
    extra["c2_pipeline_8192_scans_in_flight_scans_per_s"] = round(len(jobs_c2) / (time.perf_counter() - t0), 3)
    # BASELINE config 5 per-rank shape: 8 scans x 32768 points in lock-step, full objective + metric
    sc = sc5
    C5 = torch.from_numpy(np.stack([x[0] for x in sc])).to(dev)
    P5 = torch.from_numpy(np.stack([x[1] for x in sc])).to(dev)
    G5 = torch.from_numpy(np.stack([x[2] for x in sc])).to(dev)
    object_pose_optimization(C5, P5, radius=0.02, lr=0.01, iters=20, render_size=224)
    evaluate_scans(C5, G5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    object_pose_optimization(C5, P5, radius=0.02, lr=0.01, iters=200, render_size=224)
    evaluate_scans(C5, G5)
    torch.cuda.synchronize()
    extra["c5_rank_8x32768_registration_plus_metric_scans_per_s"] = round(8.0 / (time.perf_counter() - t0), 3)
    return extra


def cpu_baseline(a, b, budget_s=12.0):
    """Oracle Chamfer forward on all host cores, repeated until ~budget_s."""
    from oracle import oracle as O
    O.build()
    cores = O.num_threads()
    n, m = a.shape[1], b.shape[1]
    t0 = time.perf_counter()
    O.chamfer_forward(a, b, 1)
    first = time.perf_counter() - t0
    reps = max(1, min(50, int(budget_s / max(first, 1e-3))))
    t0 = time.perf_counter()
    for _ in range(reps):
        O.chamfer_forward(a, b, 1)
    dt = (time.perf_counter() - t0) / reps
    return {"value": round(2.0 * n * m / dt / 1e9, 4), "unit": "Gpair-dist/s", "cores": cores, "kind": "port",
            "sample": "oracle/genpc_oracle.c chamfer forward (OpenMP, %d threads), B=1 N=M=%d, %d calls of %.2f s"
                      % (cores, n, reps, dt)}


def cpu_context(a, b, budget_s=4.0):
    """The two other CPU routes SURVEY 8(d) names, for context beside the port (not the baseline): torch.cdist + min on all
    host threads (matmul expansion: differs from the reference's direct form at ~1e-8) and scipy's cKDTree (a pruned search:
    it does not evaluate the pairs; its rate is pairs ANSWERED per second)."""
    import torch as T
    out = {}
    n, m = a.shape[1], b.shape[1]
    try:
        ta, tb = T.from_numpy(a[0]), T.from_numpy(b[0])
        def cd():
            d = T.cdist(ta, tb)
            return d.min(1), d.min(0)
        t0 = time.perf_counter(); cd(); dt = time.perf_counter() - t0      # (a slow host: the first call is the measurement)
        if dt < budget_s / 2:
            t0 = time.perf_counter(); reps = 0
            while time.perf_counter() - t0 < budget_s and reps < 20:
                cd(); reps += 1
            dt = (time.perf_counter() - t0) / reps
        out["torch_cdist_min"] = {"gpair_s": round(2.0 * n * m / dt / 1e9, 3), "ms": round(dt * 1e3, 2), "threads": T.get_num_threads()}
    except Exception as e:
        out["torch_cdist_min"] = {"error": "%s: %s" % (type(e).__name__, e)}
    try:
        from scipy.spatial import cKDTree
        def kd():
            cKDTree(b[0]).query(a[0], k=1, workers=-1)
            cKDTree(a[0]).query(b[0], k=1, workers=-1)
        t0 = time.perf_counter(); kd(); dt = time.perf_counter() - t0
        if dt < budget_s / 2:
            t0 = time.perf_counter(); reps = 0
            while time.perf_counter() - t0 < budget_s and reps < 20:
                kd(); reps += 1
            dt = (time.perf_counter() - t0) / reps
        out["scipy_ckdtree"] = {"equivalent_gpair_s": round(2.0 * n * m / dt / 1e9, 3), "ms": round(dt * 1e3, 2),
                                "note": "tree build + query both ways, workers=-1; a pruned search: pairs answered, not evaluated"}
    except Exception as e:
        out["scipy_ckdtree"] = {"error": "%s: %s" % (type(e).__name__, e)}
    return out


def maybe_spawn(args):
    """`--gpus N` outside a torchrun environment: start the torchrun form as a CHILD process and
    exit with its code.  Runs before anything initialises a GPU (no exec from a GPU process)."""
    if args.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.exit(subprocess.call(cmd, env=env))


def synth_scan(seed, n):
    """SURVEY 8d scan bench: a complete shape (ellipsoid + box union surface, max extent 1) and a
    partial observation (the half facing the camera, resampled to n), under a similarity transform
    the registration loop can reach (scale 0.78..0.9: 201 Adam steps from 0.75)."""
    rng = np.random.default_rng(1000 + seed)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    ell = u * np.array([0.5, 0.3, 0.22])
    box = (rng.random((n, 3)) - 0.5) * np.array([0.3, 0.5, 0.3])
    face = rng.integers(0, 3, n)
    box[np.arange(n), face] = np.sign(box[np.arange(n), face]) * np.array([0.15, 0.25, 0.15])[face]
    pick = rng.random(n) < 0.6
    complete = np.where(pick[:, None], ell, box + np.array([0.1, 0.0, 0.0]))
    complete = (complete - (complete.max(0) + complete.min(0)) / 2) / (complete.max(0) - complete.min(0)).max()
    s = rng.uniform(0.78, 0.9)
    th = np.deg2rad(rng.uniform(-12, 12))
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    t = rng.uniform(-0.04, 0.04, 3)
    c = complete.mean(0)
    posed = ((complete - c) * s) @ R.T + c + t
    front = posed[posed[:, 2] > np.median(posed[:, 2]) - 0.02]
    # plain resampling -- repeated picks are EXACT copies (round 3 added noise here to dodge the NN filter's
    # tie case; the alignment loop now marks the copies once per call instead: csrc/nn_dedupe.hip)
    partial = front[rng.integers(0, front.shape[0], n)]
    return complete.astype(np.float32), partial.astype(np.float32), posed.astype(np.float32)


def scan_workload_inputs(workload, stub):
    """(total scans, points, loader(scan index) -> (complete or prediction, partial or observation, ground truth))."""
    gold = os.path.join(ROOT, "tests", "golden")
    if workload == "c3":
        # BASELINE config 3: metric.py's CD / EMD over the 13 bundled data/*.ply scans at 16384 points (committed fixture:
        # deterministic FPS subsamples, tests/golden/make_golden.py); no registration, the metric pass is the step
        z = np.load(os.path.join(gold, "scans13_fps16384.npz"))
        n = 256 if stub else 16384
        return 13, n, lambda s: (z["partial"][s][:n], None, z["gt"][s][:n])
    if workload == "c4":
        # BASELINE config 4: the 59 Waymo CAR crops at 4096 points (FPS / pad-repeat: 13 of them carry exact duplicates)
        # registered against a complete car (tests/golden/waymo_car59_4096.npz, made by make_waymo_c4.py from the
        # reference's bundled data/waymo/CAR; the reference would generate the car with Trellis)
        z = np.load(os.path.join(gold, "waymo_car59_4096.npz"))
        n = 256 if stub else 4096
        return 59, n, lambda s: (z["complete"][:n], z["crops"][s][:n], z["crops"][s][:n])
    n = 256 if stub else 32768
    return 64, n, lambda s: synth_scan(s, n)


def run_scan_workload(args, rank, world, dev):
    """BASELINE config 3 (13 bundled scans x 16384 points, CD + EMD metric), config 4 (59 Waymo crops x 4096 points over
    4 ranks) and config 5 (64 synthetic scans x 32768 points over 8 ranks): scans dealt round-robin
    (genpc_amd.sharding); c4 / c5 register per rank in lock-step groups of <= 8 (object_pose_optimization, full
    objective) and score the posed complete shape (c5: CD-L1 / CD-L2 / EMD against the ground-truth pose; c4: against
    the crop it was registered to -- a real crop has no ground truth); one all_gather of the scalars at the end.
    The line carries every rank's own elapsed time and scan count next to the MAX (load imbalance: 59 over 4, 13 over 8)."""
    from genpc_amd import sharding
    stub = os.environ.get("GENPC_BENCH_STUB") == "1"      # CI only (tests/test_sharding.py): the sharding / gather / timing path on CPU ranks, no kernels
    total, n, load = scan_workload_inputs(args.workload, stub)
    if os.environ.get("GENPC_BENCH_TOTAL"):      # measurement aid: the first k scans only (e.g. 8 = one rank's share of c5 on 8 GPUs)
        total = max(1, min(total, int(os.environ["GENPC_BENCH_TOTAL"])))
    mine = sharding.shard_indices(total, rank, world)
    scans = [load(sidx) for sidx in mine]
    register = args.workload != "c3"
    # Lock-step group size.  A rank that owns no more scans than one group of 8 (c5 on 8 GPUs: 8 scans per rank) would have
    # a single group and nothing in flight beside it: its scans are then dealt into `lanes_want` smaller groups that run
    # side by side (the first 8-GPU run should measure the configuration one would ship).
    lanes_want = max(1, int(os.environ.get("GENPC_BENCH_LANES", "3")))
    gsize = int(os.environ.get("GENPC_BENCH_GROUP", "0")) or (8 if register else 16)
    if register and not os.environ.get("GENPC_BENCH_GROUP") and 1 < len(scans) <= gsize and lanes_want > 1:
        gsize = max(2, -(-len(scans) // min(lanes_want, 2)))
    groups = []
    for g0 in range(0, len(scans), gsize):
        grp = scans[g0:g0 + gsize]
        groups.append(tuple(None if grp[0][k] is None else torch.from_numpy(np.stack([np.ascontiguousarray(x[k], np.float32) for x in grp])).to(dev)
                            for k in range(3)))

    if stub:
        def step():
            # a stand-in for registration + metric with the same shapes: per scan three scalars that depend on the
            # scan alone (so the gathered table can be checked against a single-process run)
            rows = [torch.stack([(C - G).abs().mean((1, 2)), (C - G).pow(2).mean((1, 2)), ((P if P is not None else C) - G).abs().mean((1, 2))], 1)
                    for C, P, G in groups]
            return torch.cat(rows) if rows else torch.empty(0, 3, device=dev)
    else:
        from genpc_amd.metric import evaluate_scans
        from genpc_amd.optim_registration.diff_obj_pose import object_pose_optimization

        def one(C, P, G):
            if not register:
                return evaluate_scans(C, G)
            T = torch.from_numpy(object_pose_optimization(C, P, radius=0.02, lr=0.01, iters=200, render_size=224)).to(dev)
            c = C.mean(1, keepdim=True)
            aligned = ((C - c) @ T[:, :3, :3].transpose(1, 2) + c + T[:, None, :3, 3]).contiguous()
            return evaluate_scans(aligned, G)

        # lock-step groups are independent of each other: `lanes` of them in flight (a host thread and a stream each, like
        # pipeline.complete_scans -- a group's 1800 small launches leave most of the chip idle); same rows either way
        lanes = max(1, min(int(os.environ.get("GENPC_BENCH_LANES", "3")), len(groups)))

        def step():
            if lanes == 1 or not groups:
                rows = [one(*g) for g in groups]
                return torch.cat(rows) if rows else torch.empty(0, 3, device=dev)
            from genpc_amd import pipeline
            return torch.cat(pipeline.run_in_lanes(lambda li, g: one(*g), groups, lanes, dev))

    sync = (lambda: None) if stub else torch.cuda.synchronize
    for _ in range(args.warmup):
        step()
    sync()
    sharding.barrier()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        local = step()
    sync()
    own = time.perf_counter() - t0          # this rank's own work, before it waits for the others
    sharding.barrier()
    sync()
    cdev = "cpu" if (stub or world == 1) else dev
    elapsed = sharding.max_over_ranks(time.perf_counter() - t0, device=cdev)
    table = sharding.gather_scan_metrics(local, total, rank, world)
    ranks_seen = sharding.all_ranks(cdev)
    # every rank's (scans owned, own elapsed): the same padded all_gather, one row per rank
    per_rank = sharding.gather_scan_metrics(torch.tensor([[float(len(mine)), own]], dtype=torch.float64, device=local.device),
                                            world, rank, world)
    if rank != 0:
        return None
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"scan_metrics": table.cpu().numpy()})
    what = {"c3": "CD-L1 / CD-L2 / EMD metric of the 13 bundled scans (partial vs GT), no registration",
            "c4": "diff_obj_pose registration (4 starts x 201 Adam steps, mask + 3 cd + ortho) of a complete car to each Waymo CAR "
                  "crop + CD/EMD of the posed car against the crop",
            "c5": "diff_obj_pose registration (4 starts x 201 Adam steps, mask + 3 cd + ortho) + CD/EMD metric against the true pose"}
    return {
        "metric": "completed_scans_per_s", "value": round(total * args.steps / elapsed, 4), "unit": "scans/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3),
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32",
        "data": "synthetic" if args.workload == "c5" else "reference's bundled scans (committed fixtures under tests/golden)",
        "ranks_seen": ranks_seen,
        "per_rank": [{"rank": r, "scans": int(per_rank[r, 0]), "elapsed_s": round(float(per_rank[r, 1]), 4)} for r in range(world)],
        "config": {"workload": "%s: %d scans x %d points, %s, scans sharded round-robin" % (args.workload, total, n, what[args.workload]),
                   "scans": total, "points": n, "sharding": "scan s -> rank s %% %d, all_gather of 3 scalars per scan" % world,
                   "groups_in_flight_per_rank": 1 if stub else max(1, min(int(os.environ.get("GENPC_BENCH_LANES", "3")), len(groups)))},
        "extra": {"mean_cd_l1": round(float(table[:, 0].mean()), 6), "mean_emd": round(float(table[:, 2].mean()), 6),
                  "scan_table_checksum": round(float(table.double().sum()), 9), "stub": stub},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--points", type=int, default=N_PTS)
    ap.add_argument("--workload", choices=("pairs", "c3", "c4", "c5"), default="pairs")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: per-step spread, rooflines, the oracle check, extra and cpu_baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: no cpu_baseline")
    ap.add_argument("--no-extra", action="store_true", help="with --full: no extra")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step computed as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps is None:
        args.steps = 200 if args.workload == "pairs" else 2
    if args.warmup is None:
        args.warmup = 20 if args.workload == "pairs" else 1
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    maybe_spawn(args)

    from genpc_amd import sharding
    rank, local_rank, world = sharding.init()
    if world != args.gpus:
        if rank == 0:
            print("bench.py: --gpus %d but the realised world size is %d" % (args.gpus, world), file=sys.stderr)
        sharding.shutdown()
        sys.exit(2)
    n_gpus = world
    if os.environ.get("GENPC_BENCH_STUB") == "1" and args.workload != "pairs":
        # CI only: the scan-sharded workloads' control path on CPU ranks over gloo (no kernel runs, nothing is measured)
        out = run_scan_workload(args, rank, world, torch.device("cpu"))
        if rank == 0:
            print(json.dumps(out), flush=True)
        sharding.shutdown()
        return
    assert torch.cuda.is_available(), "bench.py needs a GPU (the HIP path has no fallback)"
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    if args.workload != "pairs":
        out = run_scan_workload(args, rank, world, dev)
        if rank == 0:
            print(json.dumps(out), flush=True)
        sharding.shutdown()
        return

    from genpc_amd import _lib, chamfer_3D

    n = args.points
    A, B, a_np, b_np = make_pair(n, SEED + rank, dev)
    dist1 = torch.empty(1, n, device=dev)
    dist2 = torch.empty(1, n, device=dev)
    idx1 = torch.empty(1, n, device=dev, dtype=torch.int32)
    idx2 = torch.empty(1, n, device=dev, dtype=torch.int32)
    stream = torch.cuda.current_stream(dev)

    def step():
        rc = chamfer_3D.forward(A, B, dist1, dist2, idx1, idx2)
        if rc != 1:
            raise RuntimeError("chamfer forward failed: " + _lib.last_error())

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    sharding.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    sharding.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    # what the last timed step computed, copied on the launch stream before any later step (--full) overwrites it
    last = {"dist1": dist1.clone(), "dist2": dist2.clone(), "idx1": idx1.clone(), "idx2": idx2.clone()} if args.dump_outputs else None
    elapsed = sharding.max_over_ranks(elapsed, device=dev if world > 1 else "cpu")
    ranks_seen = sharding.all_ranks(dev if world > 1 else "cpu")

    pairs_per_step = 2.0 * n * n
    value = n_gpus * pairs_per_step * args.steps / elapsed / 1e9

    out = None
    if rank == 0:
        out = {
            "metric": "chamfer_nn_pair_dist_throughput",
            "value": round(value, 3),
            "unit": "Gpair-dist/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 5),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "ranks_seen": ranks_seen,
            "config": {"workload": "chamfer_3DDist.forward B=1 N=M=%d (both directions), one pair per rank" % n,
                       "points": n, "batch": 1, "arith": "fma" if _lib.lib.genpc_get_arith() else "strict",
                       "sharding": "independent scans per rank, no data-path collective"},
        }
    if rank == 0 and args.full:
        # ---- per-step spread and the dominant kernel's own duration: HIP events on the launch stream, taken right
        # after the timed region (before any host-side checker work disturbs the launch thread)
        reps = max(20, min(args.steps, 200))
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        evs[0].record(stream)
        for k in range(reps):
            step()
            evs[k + 1].record(stream)
        evs[-1].synchronize()
        per_step = sorted(evs[k].elapsed_time(evs[k + 1]) for k in range(reps))
        ms = evs[0].elapsed_time(evs[-1]) / reps
        # the filter kernel alone: HIP events inside the library, on the launch stream
        _lib.lib.genpc_nn_profile(1)
        kms = []
        for _ in range(reps):
            step()
            kms.append(float(_lib.lib.genpc_nn_profile(1)))
        _lib.lib.genpc_nn_profile(0)
        kms = [k for k in kms if k > 0]
        kernel_ms = sum(kms) / len(kms) if kms else ms
        kernel_name = "nn_f16_kernel" if kms else "nn step (filter kernel not in use)"
        step()
        torch.cuda.synchronize()
        # the timed step's output against the oracle (checker only): first and last 256 queries of
        # each direction, every distance and index
        from oracle import oracle as O
        sel = np.r_[0:256, n - 256:n]
        e1, _, j1, _ = O.chamfer_forward(a_np[:, sel], b_np, 1)
        e2, _, j2, _ = O.chamfer_forward(b_np[:, sel], a_np, 1)
        ok = (np.array_equal(dist1.cpu().numpy()[:, sel], e1) and np.array_equal(idx1.cpu().numpy()[:, sel], j1)
              and np.array_equal(dist2.cpu().numpy()[:, sel], e2) and np.array_equal(idx2.cpu().numpy()[:, sel], j2))
        if not ok:
            raise RuntimeError("bench.py: the timed step's output differs from the oracle")
        tflops = MFMA_FLOP_PER_PAIR * pairs_per_step / (kernel_ms * 1e-3) / 1e12
        alg_bytes = 20.0 * (n + n)        # 12 B read + 8 B written per point, both clouds
        out.update({
            "ms_per_step_spread": {"min": round(per_step[0], 5), "median": round(per_step[len(per_step) // 2], 5),
                                   "max": round(per_step[-1], 5), "steps": len(per_step),
                                   "how": "HIP events between consecutive steps, a second pass right after the timed region"},
            "output_checked": "first and last 256 queries of both directions (512 of 16384 each) bit-exact vs the oracle inside this run; every distance and index of the same input: tests/test_gpu_chamfer_parity.py::test_bench_input_elementwise (-m gpu)",
            "roofline": {"bound": "mfma", "achieved": round(tflops, 3), "peak": PEAK_F16_MFMA_TFLOPS,
                         "unit": "TFLOP/s", "frac": round(tflops / PEAK_F16_MFMA_TFLOPS, 4), "traffic": None,
                         "kernel": kernel_name, "ms_per_launch": round(kernel_ms, 5),
                         "flop_per_pair": MFMA_FLOP_PER_PAIR, "mfma_dtype": "f16",
                         "step_ms_events": round(ms, 5),
                         # SURVEY 8d's definition for a1: 8 algorithmic flop per pair over the WHOLE step against the
                         # fp32 vector peak (the pair evaluation itself runs on the f16 matrix pipe: this is an
                         # equivalent rate, "~0.5 is the practical maximum" for a VALU kernel)
                         "step_frac_fp32_valu": round(FLOP_PER_PAIR * pairs_per_step / (elapsed / args.steps) / 1e12 / PEAK_FP32_TFLOPS, 4)},
            "roofline_hbm": {"bound": "hbm", "achieved": round(alg_bytes / (ms * 1e-3) / 1e9, 3),
                             "peak": PEAK_HBM_GBS, "unit": "GB/s",
                             "frac": round(alg_bytes / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS, 6), "traffic": None,
                             "algorithmic_bytes": alg_bytes},
        })
        out["roofline"]["traffic"], out["roofline"]["traffic_source"] = pmc_traffic(n)
    # the last collective: the other ranks leave here; rank 0's secondary measurements and the CPU baseline run
    # AFTER it (nobody waits in RCCL for them)
    sharding.barrier()
    sharding.shutdown()
    if rank == 0:
        # (the headline above is measured and complete: nothing below may keep the line from being printed)
        if args.full and not args.no_extra:
            try:
                out["extra"] = extras(A, B, n, dev, stream)
            except Exception as e:
                out["extra"] = {"error": "%s: %s" % (type(e).__name__, e)}
        if args.full and not args.no_cpu_baseline:
            try:
                out["cpu_baseline"] = cpu_baseline(a_np, b_np)
            except Exception as e:
                out["cpu_baseline"] = {"value": None, "error": "%s: %s" % (type(e).__name__, e)}
            if isinstance(out.get("extra"), dict) and "error" not in out["extra"]:
                out["extra"]["cpu_context_16384x16384"] = cpu_context(a_np, b_np)
        if last is not None:
            dump_outputs(args.dump_outputs, {k: v.cpu().numpy() for k, v in last.items()})
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
