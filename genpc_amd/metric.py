"""Evaluation harness with the arithmetic of the reference's ``main.metric``
(main.py:11-36): CD-L1 and EMD(eps 0.005, 50 rounds) between a completed cloud and
its ground truth, printed x100.  The reference does this one scan at a time after
reading PLY files with open3d and subsampling with fpsample (random start, not
reproducible); here the clouds arrive as tensors (fixtures are deterministic-FPS
subsamples, tests/golden/make_golden.py), scans are batched per call and sharded
over ranks (genpc_amd.sharding) with one all_gather of the per-scan scalars.

    python -m genpc_amd.metric [--npz tests/golden/scans13_fps16384.npz]
    torchrun --nproc-per-node 4 -m genpc_amd.metric --npz ...

The reference's second evaluation file, ``metric.py``, adds what needs no ground truth: ``UHD`` (:105-132), the directed
Hausdorff distance from the partial scan to the completed cloud -- the one score of the LiDAR path -- and ``cd_emd``
(:135-148).  ``uhd`` / ``UHD`` / ``evaluate_uhd`` / ``cd_emd`` below; UHD runs on the library's fp64 all-pairs kernel
(csrc/uhd.hip) and has the bits of scipy's float64 ``cdist``.  ``mesh_cd_emd`` is the tensor form of its evaluation of a
reconstructed mesh against a ground-truth MESH (``metric_sds_redwood``, :49-94), both sampled on the device.

    python -m genpc_amd.metric --uhd PARTIAL.ply COMPLETE.ply

``evaluate_clouds`` is ``evaluate_scans`` for clouds of different sizes -- what ``metric_my_redwood(flag, cd_l1=True)``
(metric.py:10-48) scores one file at a time: a prediction against a ground truth of whatever size its file has -- on the
ragged nearest-neighbour search (csrc/nn_ragged.hip), all scans in one call per direction.

    python -m genpc_amd.metric --clouds PRED_DIR GT_DIR

``uhd_ragged`` is ``uhd`` for S (partial, complete) pairs of different sizes in one library call (csrc/uhd_ragged.hip) --
the reference applies ``UHD`` to a list of scans one file pair at a time and averages (metric.py:182-195) -- with the same
float64 bits per pair; ``score_uhd_folders`` reads two folders of PLY files under ``UHD``'s thresholds and scores all pairs
at once.

    python -m genpc_amd.metric --uhd-dirs PARTIAL_DIR COMPLETE_DIR

``evaluate_scans_ragged`` is ``evaluate_scans`` -- CD-L1, CD-L2 and EMD -- for S scans of different sizes, scan j with the
same N_j points (a multiple of 256) on both sides: ``evaluate_clouds``' two columns plus one ragged auction call
(csrc/emd_ragged.hip) for all scans.
"""
import argparse
import os

import numpy as np
import torch

from . import _lib, sharding
from .loss_functions import chamfer_3DDist, emdModule


def evaluate_scans(pred, gt, eps=0.005, iters=50):
    """pred, gt: [S,N,3] GPU tensors (N % 256 == 0).  Returns [S,3] = CD-L1, CD-L2,
    EMD per scan, with the reductions of utils/loss_util.py:25-49 applied per scan."""
    d1, d2, _, _ = chamfer_3DDist()(pred, gt)
    cd_l1 = (torch.sqrt(d1).mean(1) + torch.sqrt(d2).mean(1)) / 2
    cd_l2 = d1.mean(1) + d2.mean(1)
    de, _ = emdModule()(pred, gt, eps, iters)
    emd = torch.sqrt(de).mean(1)
    return torch.stack([cd_l1, cd_l2, emd], dim=1)


def evaluate_clouds(preds, gts):
    """preds, gts: S clouds each, of any sizes -- lists of [N_j,3] / [M_j,3] float32 GPU tensors, or packed as (points,
    offsets) (loss_functions/Chamfer3D/dist_chamfer_ragged.py).  Returns float64 [S,2] = CD-L1, CD-L2 per scan with the
    reductions of utils/loss_util.py:25-33: sqrt in fp32 as there, each scan's means accumulated in float64 over its own
    segment.  No EMD column: the auction needs equal sizes.  Stays on the device; a scan with an empty cloud scores NaN."""
    from .loss_functions.Chamfer3D.dist_chamfer_ragged import chamfer_ragged
    d1, d2, _, _, off1, off2 = chamfer_ragged(preds, gts)
    s = off1.numel() - 1

    def seg_means(d, off):
        counts = (off[1:] - off[:-1]).to(d.device)
        seg = torch.repeat_interleave(torch.arange(s, device=d.device), counts, output_size=d.numel())
        cnt = counts.double()
        m1 = torch.zeros(s, dtype=torch.float64, device=d.device).index_add_(0, seg, torch.sqrt(d).double()) / cnt
        m2 = torch.zeros(s, dtype=torch.float64, device=d.device).index_add_(0, seg, d.double()) / cnt
        return m1, m2
    a1, a2 = seg_means(d1, off1)
    b1, b2 = seg_means(d2, off2)
    return torch.stack([(a1 + b1) / 2, a2 + b2], dim=1)


def evaluate_scans_ragged(preds, gts, eps=0.005, iters=50):
    """``evaluate_scans`` for S scans of different sizes: preds, gts as ``evaluate_clouds`` takes them, scan j with N_j points
    on BOTH sides, N_j % 256 == 0 (the auction's rule).  Returns float64 [S,3] on the device: columns 0-1 are
    ``evaluate_clouds``'s CD-L1 and CD-L2, column 2 the EMD of ``evaluate_scans`` (eps, iters) from ONE ragged auction call
    (csrc/emd_ragged.hip) -- the float64 mean of the float64 square roots of the scan's fp32 dist.  Forward only."""
    from .loss_functions.Chamfer3D.dist_chamfer_ragged import pack_clouds
    from .loss_functions.emd.emd_ragged import check_pairs, forward_packed
    p1, off1 = pack_clouds(preds, "preds")
    p2, off2 = pack_clouds(gts, "gts")
    check_pairs(off1, off2, "evaluate_scans_ragged")
    _lib.require_gpu(p1, p2)
    cd = evaluate_clouds((p1, off1), (p2, off2))
    s = len(off1) - 1
    with torch.no_grad():
        dist = forward_packed(p1.detach(), p2.detach(), off1, eps, iters)["dist"]
    counts = torch.tensor([b - a for a, b in zip(off1, off1[1:])], dtype=torch.int64).to(dist.device)
    seg = torch.repeat_interleave(torch.arange(s, device=dist.device), counts, output_size=dist.numel())
    emd = torch.zeros(s, dtype=torch.float64, device=dist.device).index_add_(0, seg, torch.sqrt(dist.double())) / counts.double()
    return torch.cat([cd, emd[:, None]], dim=1)


def match_cloud_files(pred_dir, gt_dir):
    """The PLY files of two folders matched by file name: (pairs, only_pred, only_gt) with pairs = [(name, pred path,
    gt path)] in name order and the names that lack a counterpart on either side.  Touches no GPU."""
    def plys(d):
        return {f for f in os.listdir(d) if f.lower().endswith(".ply") and os.path.isfile(os.path.join(d, f))}
    p, g = plys(pred_dir), plys(gt_dir)
    pairs = [(f, os.path.join(pred_dir, f), os.path.join(gt_dir, f)) for f in sorted(p & g)]
    return pairs, sorted(p - g), sorted(g - p)


def score_cloud_folders(pred_dir, gt_dir):
    """CD-L1 and CD-L2 of every PLY of pred_dir against the PLY of the same name in gt_dir, at the files' own sizes:
    (names, float64 [S,2] on the host, only_pred, only_gt)."""
    from .utils.dataUtils import read_ply
    pairs, only_pred, only_gt = match_cloud_files(pred_dir, gt_dir)
    dev = torch.device("cuda", torch.cuda.current_device())

    def load(path):
        xyz, _ = read_ply(path, want_color=False)
        return torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float32)).reshape(-1, 3).to(dev)
    if not pairs:
        return [], np.zeros((0, 2)), only_pred, only_gt
    table = evaluate_clouds([load(p) for _, p, _ in pairs], [load(g) for _, _, g in pairs])
    return [n for n, _, _ in pairs], table.cpu().numpy(), only_pred, only_gt


def cd_l1_cpu_plumbing(pred, gt, chunk=512):
    """BASELINE config 1: CD-L1 of CPU tensors in plain torch -- the metric's plumbing without a GPU.  NOT a
    fallback: nothing in the library routes here (CPU tensors handed to chamfer_3DDist / emdModule raise); a caller that
    wants the CPU number asks for it by name (``python -m genpc_amd.metric --cpu``).  Direct form in the reference's
    operation order, fp32: d = ((x2-x1)^2 + (y2-y1)^2) + (z2-z1)^2, min over the other cloud, then
    (mean sqrt d1 + mean sqrt d2) / 2 (utils/loss_util.py:25-29).  pred, gt: [S,N,3] / [S,M,3] float32 CPU."""
    if pred.is_cuda or gt.is_cuda:
        raise ValueError("cd_l1_cpu_plumbing is the CPU plumbing path; GPU tensors go through evaluate_scans")
    pred, gt = pred.float(), gt.float()

    def one_way(a, b):                      # [N,3] x [M,3] -> [N] squared NN distances
        out = []
        for i in range(0, a.shape[0], chunk):
            d = b[None, :, :] - a[i:i + chunk, None, :]
            out.append(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).min(1).values)
        return torch.cat(out)
    rows = [(torch.sqrt(one_way(p, g)).mean() + torch.sqrt(one_way(g, p)).mean()) / 2 for p, g in zip(pred, gt)]
    return torch.stack(rows)


def _uhd_cloud(t, name):
    """A cloud as contiguous float32.  float64 is taken only if every value survives the trip through float32 (checked on the
    device): PLY clouds are float32 that open3d widens, and the kernel widens them again, so nothing is lost; a genuinely
    float64 cloud would be answered for different coordinates than the caller's, and is refused."""
    if t.dtype == torch.float64:
        t32 = t.float()
        if not bool((t32.double() == t).all()):
            raise ValueError("uhd: %s is float64 and not representable in float32 (the kernel reads float32 coordinates)" % name)
        t = t32
    elif t.dtype != torch.float32:
        raise TypeError("uhd: %s must be torch.float32 (or float32-representable float64), got %s" % (name, t.dtype))
    return t.contiguous()


def uhd(partial, complete, return_witness=False):
    """Directed Hausdorff distance from ``partial`` to ``complete``: max over the points of partial of the distance to the
    nearest point of complete, with the bits of the reference's ``np.max(np.min(cdist(partial, complete), axis=1))``
    (metric.py:124-130; float64, ((dx*dx) + (dy*dy)) + (dz*dz), one sqrt).  [B,N,3] with [B,M,3] -> float64 [B]; [N,3] with
    [M,3] -> a 0-d float64 tensor; float32 GPU tensors (float64 only if float32-representable).  The result stays on the
    device: nothing here waits for it (a float64 input costs one synchronising check).

    return_witness=True also returns int32 [B,2] (or [2]): (i, j) = numpy's ``argmax`` of the row minima and ``argmin`` of
    that row -- the lowest indices among ties, judged on the float64 squared distances."""
    if partial.dim() != complete.dim() or partial.dim() not in (2, 3) or partial.shape[-1] != 3 or complete.shape[-1] != 3:
        raise ValueError("uhd: partial [N,3] with complete [M,3], or [B,N,3] with [B,M,3]")
    single = partial.dim() == 2
    p = partial.unsqueeze(0) if single else partial
    c = complete.unsqueeze(0) if single else complete
    if p.shape[0] != c.shape[0]:
        raise ValueError("uhd: batch sizes differ (%d, %d)" % (p.shape[0], c.shape[0]))
    if p.device != c.device:
        raise ValueError("uhd: partial and complete are on different devices")
    b, n, m = p.shape[0], p.shape[1], c.shape[1]
    if n < 1 or m < 1:
        raise ValueError("uhd: the maximum or minimum over an empty cloud is undefined (N = %d, M = %d)" % (n, m))
    p, c = _uhd_cloud(p, "partial"), _uhd_cloud(c, "complete")      # (the dtype is judged where the tensor lives)
    _lib.require_gpu(p, c)
    d2 = torch.empty((b,), dtype=torch.float64, device=p.device)
    ij = torch.empty((b, 2), dtype=torch.int32, device=p.device)
    if b:
        rc = _lib.on_device_of(p, _lib.lib.genpc_uhd, b, n, _lib.ptr(p), m, _lib.ptr(c), _lib.ptr(d2), _lib.ptr(ij))
        if rc != 0:
            raise RuntimeError("genpc_uhd failed (%d): %s" % (rc, _lib.last_error()))
    hd = torch.sqrt(d2)
    if single:
        hd, ij = hd[0], ij[0]
    return (hd, ij) if return_witness else hd


def _read_cloud(path, fps_at, fps_to, device):
    """A PLY's points on the device; a cloud of >= fps_at points is farthest-point-subsampled to fps_to through float32
    (metric.py:117-122)."""
    from .fps import fps_subsample
    from .utils.dataUtils import read_ply
    xyz, _ = read_ply(path, want_color=False)
    t = torch.from_numpy(np.ascontiguousarray(xyz)).to(device)
    if fps_at is not None and len(xyz) >= fps_at:
        t = fps_subsample(t.unsqueeze(0).float().contiguous(), fps_to).squeeze(0)
    return t


def UHD(partial_path, complete_path):
    """The reference's ``UHD(partial_path, complete_path)`` (metric.py:105-132), same signature and thresholds: both PLY
    clouds are read, one with >= 20000 points is FPS-subsampled (through float32) to 10000 (partial) / 20000 (complete)
    points, and the directed Hausdorff distance partial -> complete comes back as a Python float.

    Below the threshold the result has the reference's bits (``uhd``).  At or above it the reference's ``fps_subsample``
    starts at a random point and is not reproducible from run to run; ours (genpc_amd.fps) is deterministic, so that branch
    returns the same number every time and is not pinned to the reference."""
    dev = torch.device("cuda", torch.cuda.current_device())
    p = _read_cloud(partial_path, 20000, 10000, dev)
    c = _read_cloud(complete_path, 20000, 20000, dev)
    return float(uhd(p, c))


UHD_RAGGED_MAX_PAIRS = 384          # include/genpc_hip.h: pairs per genpc_uhd_ragged call


def _uhd_ragged_side(clouds, name):
    """One side of a ragged UHD batch as (points [T,3] float32 contiguous, offsets: S + 1 Python ints): a list of [N_j,3]
    tensors or packed (points, offsets), as pack_clouds reads them, each cloud under _uhd_cloud's dtype rule."""
    from ._ragged import is_packed, pack_clouds
    if is_packed(clouds):
        points, off = clouds
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError("uhd_ragged: packed %s must be [T,3], got %s" % (name, tuple(points.shape)))
        return pack_clouds((_uhd_cloud(points, name), off), name)
    if not isinstance(clouds, (list, tuple)):
        raise TypeError("uhd_ragged: %s is a list of [N,3] tensors or a tuple (points, offsets)" % name)
    for j, t in enumerate(clouds):
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError("uhd_ragged: %s[%d] must be an [N,3] tensor" % (name, j))
    return pack_clouds([_uhd_cloud(t, "%s[%d]" % (name, j)) for j, t in enumerate(clouds)], name)


def uhd_ragged(partials, completes, return_witness=False):
    """``uhd`` for S pairs of clouds of any sizes: pair j is partials[j] [N_j,3] against completes[j] [M_j,3].  Each side is
    a list of float32 GPU tensors (float64 only if float32-representable, as for ``uhd``) or packed as (points [T,3],
    offsets) -- S + 1 host ints, ``pack_clouds`` of loss_functions/Chamfer3D/dist_chamfer_ragged.py.  Returns float64 [S] on
    the device, per pair the bits of ``uhd`` on that pair alone; return_witness=True also returns int32 [S,2], (i, j) counted
    inside the pair's own clouds.  One library call per 384 pairs (genpc_uhd_ragged; a longer list takes several), nothing
    waits for the result (a float64 input costs one synchronising check per tensor).  An empty cloud is an error."""
    from ._ragged import chunks, host_ints
    p, poff = _uhd_ragged_side(partials, "partials")
    c, coff = _uhd_ragged_side(completes, "completes")
    if len(poff) != len(coff):
        raise ValueError("uhd_ragged: %d partial clouds against %d complete clouds" % (len(poff) - 1, len(coff) - 1))
    s = len(poff) - 1
    for j in range(s):
        n, m = poff[j + 1] - poff[j], coff[j + 1] - coff[j]
        if n < 1 or m < 1:
            raise ValueError("uhd_ragged: pair %d has an empty cloud (N = %d, M = %d): the maximum or minimum over an empty "
                             "cloud is undefined" % (j, n, m))
    if s == 0:
        dev = p.device if p.is_cuda else (c.device if c.is_cuda else torch.device("cuda", torch.cuda.current_device()))
        hd, ij = torch.empty((0,), dtype=torch.float64, device=dev), torch.empty((0, 2), dtype=torch.int32, device=dev)
        return (hd, ij) if return_witness else hd
    _lib.require_gpu(p, c)
    if p.device != c.device:
        raise ValueError("uhd_ragged: partials and completes are on different devices")
    d2 = torch.empty((s,), dtype=torch.float64, device=p.device)
    ij = torch.empty((s, 2), dtype=torch.int32, device=p.device)
    for a, b, na, ma in chunks(UHD_RAGGED_MAX_PAIRS, poff, coff):
        rc = _lib.on_device_of(p, _lib.lib.genpc_uhd_ragged, b - a, host_ints(na, "noff")[1], _lib.ptr(p[poff[a]:poff[b]]),
                               host_ints(ma, "moff")[1], _lib.ptr(c[coff[a]:coff[b]]), _lib.ptr(d2[a:b]), _lib.ptr(ij[a:b]))
        if rc != 0:
            raise RuntimeError("genpc_uhd_ragged failed (%d): %s" % (rc, _lib.last_error()))
    hd = torch.sqrt(d2)
    return (hd, ij) if return_witness else hd


def score_uhd_folders(partial_dir, complete_dir):
    """``UHD`` of every PLY of partial_dir against the PLY of the same name in complete_dir, all pairs in one ragged call:
    (names, float64 [S] on the host, only_partial, only_complete).  Each file is read as ``UHD`` reads it -- a cloud of
    >= 20000 points is FPS-subsampled to 10000 (partial) / 20000 (complete) -- so entry j is the float ``UHD`` returns for
    pair j."""
    pairs, only_partial, only_complete = match_cloud_files(partial_dir, complete_dir)
    if not pairs:
        return [], np.zeros((0,)), only_partial, only_complete
    dev = torch.device("cuda", torch.cuda.current_device())
    hd = uhd_ragged([_read_cloud(p, 20000, 10000, dev) for _, p, _ in pairs], [_read_cloud(c, 20000, 20000, dev) for _, _, c in pairs])
    return [n for n, _, _ in pairs], hd.cpu().numpy(), only_partial, only_complete


def cd_emd(pcdpath1, pcdpath2):
    """The reference's ``cd_emd`` (metric.py:135-148): both PLY clouds FPS-subsampled to 16384 points, then CD-L1 with
    gen = cloud 2, gt = cloud 1 and EMD (eps 0.005, 50 rounds) with p1 = cloud 2, p2 = cloud 1.  Returns the two 0-d
    tensors (cdloss, emdloss)."""
    from .fps import fps_subsample
    from .utils.dataUtils import read_ply
    from .utils.loss_util import Completionloss
    dev = torch.device("cuda", torch.cuda.current_device())
    clouds = []
    for path in (pcdpath1, pcdpath2):
        xyz, _ = read_ply(path, want_color=False)
        t = torch.from_numpy(np.ascontiguousarray(xyz)).unsqueeze(0).float().to(dev)
        clouds.append(fps_subsample(t.contiguous(), 16384).float())
    pcd1, pcd2 = clouds
    cdloss = Completionloss(loss_func='cd_l1').get_loss(gen=pcd2, gt=pcd1)
    emdloss = Completionloss(loss_func='emd').emd_loss(p1=pcd2, p2=pcd1)
    return cdloss, emdloss


def mesh_cd_emd(gt_vertices, gt_faces, est_vertices, est_faces, seed=0, samples=40000, points=16384):
    """The reference's evaluation of an estimated mesh against a ground-truth mesh (metric.py:49-94) on tensors: both meshes
    are translated by the GT's bounding-box centre and scaled by 1 / max(GT extent) (:50-61), each is sampled `samples`
    times on its surface (:64-65; here on the device, utils/mesh_io.sample_surface_gpu, reproducible from `seed`), both
    samplings are FPS-subsampled to `points` (:82-87), then CD-L1 and EMD with gen = est, gt = GT (:89-92).  Returns the
    two 0-d tensors (cdloss, emdloss).  vertices / faces: GPU tensors or numpy arrays.  seed: an int -- both meshes draw
    the same random words -- or a pair (gt_seed, est_seed).  The reference's visualisation cloud, plane file and OBJ
    reading (:59,66-81) are not part of it."""
    from .fps import fps_subsample
    from .utils.loss_util import Completionloss
    from .utils.mesh_io import _device_array, sample_surface_gpu
    seeds = tuple(seed) if isinstance(seed, (tuple, list)) else (seed, seed)
    if len(seeds) != 2:
        raise ValueError("mesh_cd_emd: seed is an int or a pair (gt_seed, est_seed)")
    given = [t for t in (gt_vertices, est_vertices) if torch.is_tensor(t) and t.is_cuda]
    dev = given[0].device if given else torch.device("cuda", torch.cuda.current_device())
    gv = _device_array(gt_vertices, torch.float32, dev, "gt_vertices")
    ev = _device_array(est_vertices, torch.float32, dev, "est_vertices")
    lo, hi = gv.double().min(0).values, gv.double().max(0).values
    center, scale = (lo + hi) / 2, 1.0 / (hi - lo).max()
    clouds = []
    for v, f, sd in ((gv, gt_faces, seeds[0]), (ev, est_faces, seeds[1])):
        v = ((v.double() - center) * scale).float()                     # :56-57, :60-61 (open3d moves doubles)
        pts, _ = sample_surface_gpu(v, f, samples, sd, device=dev)
        clouds.append(fps_subsample(pts.unsqueeze(0).contiguous(), points).float())
    gt, est = clouds
    cdloss = Completionloss(loss_func='cd_l1').get_loss(gen=est, gt=gt)
    emdloss = Completionloss(loss_func='emd').get_loss(gen=est, gt=gt)
    return cdloss, emdloss


def evaluate_uhd(pred, gt):
    """metric_fn for evaluate_sharded: pred [S,N,3] are the partial scans (queries), gt [S,M,3] the completed clouds
    (targets).  Returns float64 [S,1] = uhd(pred, gt); the all-gather keeps the dtype."""
    return uhd(pred, gt).unsqueeze(1)


def evaluate_sharded(pred_np, gt_np, device=None, max_batch=16, metric_fn=None, backend=None):
    """Round-robin shard of the S scans over the ranks of the default process group
    (initialised here if the launcher's WORLD_SIZE > 1 and nobody did yet); every rank
    returns the full [S,K] table (scan order).  metric_fn(pred[S',N,3], gt[S',N,3]) ->
    [S',K] defaults to evaluate_scans (K = 3: CD-L1, CD-L2, EMD)."""
    rank, local_rank, world = sharding.init(backend)
    if metric_fn is None:
        metric_fn = evaluate_scans
    if device is None:
        device = torch.device("cuda", local_rank)
    s_total = pred_np.shape[0]
    mine = sharding.shard_indices(s_total, rank, world)
    rows = []
    for i in range(0, len(mine), max_batch):
        sel = mine[i:i + max_batch]
        p = torch.from_numpy(np.ascontiguousarray(pred_np[sel])).to(device)
        g = torch.from_numpy(np.ascontiguousarray(gt_np[sel])).to(device)
        rows.append(metric_fn(p, g))
    # K (columns per scan) is agreed on collectively: a rank that owns no scan (more ranks than scans) cannot know
    # what a custom metric_fn returns, and ranks entering the all_gather with different shapes would hang
    k_local = rows[0].shape[1] if rows else 0
    k = int(sharding.max_over_ranks(float(k_local), device=device if (world > 1 and torch.device(device).type == "cuda") else "cpu"))
    if k <= 0:
        raise ValueError("evaluate_sharded: no rank owns a scan")
    if rows and any(r.shape[1] != k for r in rows):
        raise ValueError("evaluate_sharded: metric_fn returned %d columns here, %d elsewhere" % (k_local, k))
    # ... and so is the dtype (evaluate_uhd returns float64): the all_gather needs one on every rank
    red_dev = device if (world > 1 and torch.device(device).type == "cuda") else "cpu"
    wide = sharding.max_over_ranks(1.0 if rows and rows[0].dtype == torch.float64 else 0.0, device=red_dev) > 0
    local = torch.cat(rows) if rows else torch.empty(0, k, device=device, dtype=torch.float64 if wide else torch.float32)
    return sharding.gather_scan_metrics(local, s_total, rank, world)


def main():
    ap = argparse.ArgumentParser()
    here = os.path.dirname(os.path.abspath(__file__))
    ap.add_argument("--npz", default=os.path.join(here, "..", "tests", "golden", "scans13_fps16384.npz"))
    ap.add_argument("--cpu", action="store_true", help="BASELINE config 1: CD-L1 only, plain torch on the CPU (plumbing, no GPU)")
    ap.add_argument("--uhd", nargs=2, metavar=("PARTIAL.ply", "COMPLETE.ply"),
                    help="directed Hausdorff distance partial -> complete of two PLY clouds (the reference's UHD), printed x100")
    ap.add_argument("--clouds", nargs=2, metavar=("PRED_DIR", "GT_DIR"),
                    help="CD-L1 of every PLY of PRED_DIR against the PLY of the same name in GT_DIR, at the files' own sizes, printed x100")
    ap.add_argument("--uhd-dirs", nargs=2, metavar=("PARTIAL_DIR", "COMPLETE_DIR"),
                    help="UHD of every PLY of PARTIAL_DIR against the PLY of the same name in COMPLETE_DIR, all pairs in one call, and their mean, printed x100")
    args = ap.parse_args()
    if args.uhd_dirs:
        names, hds, only_partial, only_complete = score_uhd_folders(*args.uhd_dirs)
        total = 0
        for name, hd in zip(names, hds):
            hd = float(hd)
            print(f"{name} : {hd * 100:.2f}")
            total += hd                                                               # metric.py:193
        for side, lost in (("COMPLETE_DIR", only_partial), ("PARTIAL_DIR", only_complete)):
            for name in lost:
                print(f"{name} : no counterpart in {side}")
        if names:
            print(f"UHD: {total / len(names) * 100:.2f}")                             # metric.py:194-195
        return
    if args.clouds:
        names, table, only_pred, only_gt = score_cloud_folders(*args.clouds)
        for name, (cd, _) in zip(names, table):
            print(f"{name} : {cd * 100:.2f}")                                       # metric.py:40
        for side, lost in (("GT_DIR", only_pred), ("PRED_DIR", only_gt)):
            for name in lost:
                print(f"{name} : no counterpart in {side}")
        return
    if args.uhd:
        print(f"UHD: {UHD(*args.uhd) * 100:.2f}")                                   # metric.py:195
        return
    if args.cpu:
        z = np.load(args.npz)
        cd = cd_l1_cpu_plumbing(torch.from_numpy(z["partial"]), torch.from_numpy(z["gt"]))
        ids = z["ids"] if "ids" in z.files else [str(i) for i in range(len(cd))]
        for flag, v in zip(ids, cd):
            print(f"Flag: {flag}, CD: {float(v) * 100:.3f}")
        return
    rank, local_rank, world = sharding.init()
    torch.cuda.set_device(local_rank)
    z = np.load(args.npz)
    table = evaluate_sharded(z["partial"], z["gt"]).cpu().numpy()
    if rank == 0:
        for flag, (cd, _, emd) in zip(z["ids"], table):
            print(f"Flag: {flag}, CD: {cd * 100:.3f}, EMD: {emd * 100:.3f}")      # main.py:35
        ok = [i for i, f in enumerate(z["ids"]) if f != "06830"]                  # GT mis-framed
        print(f"mean over {len(ok)} well-framed scans: CD {table[ok, 0].mean() * 100:.6f} "
              f"EMD {table[ok, 2].mean() * 100:.6f}")
    sharding.shutdown()


if __name__ == "__main__":
    main()
