"""ICP + scale search of the reference's ``reg_xyz.py`` on the gfx950 library
(SURVEY.md 8a row a17): ``icp_with_scaling`` (:24-38), ``icp_with_scaling_xyz``
(:9-21), the coarse 11-scale sweep of ``reg`` (:146-173) and
``iterative_scale_search`` (:60-96).  Same names, argument meaning and returned
quantities; clouds are [N,3] GPU tensors (the reference passes open3d point clouds;
open3d is absent and unpinned -- see DESIGN.md).  Voxel down-sampling, noise
removal and the fusion tail of ``reg`` are the "next" rows of SURVEY 8f.

Batching: the 11 coarse candidates share their first ICP (it does not depend on
the scale) and run their second ICP as one K=11 batch; the 10x10x10 anisotropic
search scores all 1000 candidates with one batched NN launch and solves ICP only
for the winner, because the reference's score (:77-83) is computed on the scaled
source, before and independently of the candidate's ICP result.
"""
import numpy as np
import torch

from . import _lib
from ._ragged import chunks, host_ints, ragged_side
from .loss_functions import chamfer_3DDist

_L = _lib.lib
_p = _lib.ptr


def registration_icp(source, target, max_correspondence_distance, init=None, max_iteration=30,
                     relative_fitness=1e-6, relative_rmse=1e-6):
    """open3d.pipelines.registration.registration_icp(point-to-point) for K initial
    transforms at once.  init: [4,4] or [K,4,4] (numpy / tensor, float64).
    Returns (transformation [K,4,4] float64 numpy, fitness [K], inlier_rmse [K], iters [K]);
    a single [4,4] init returns unbatched values."""
    source = source.contiguous().float()
    target = target.contiguous().float()
    _lib.check_tensors((("source", source), ("target", target)))
    dev = source.device
    if init is None:
        init = np.eye(4)
    init_t = torch.as_tensor(np.asarray(init, np.float64)).reshape(-1, 4, 4).contiguous().to(dev)
    k = init_t.shape[0]
    buf = torch.empty(k * 19, dtype=torch.float64, device=dev)          # transforms and statistics: one copy back
    out_T, stats = buf[:k * 16], buf[k * 16:]
    rc = _lib.on_device_of(source, _L.genpc_icp_batch, k, source.shape[0], _p(source), target.shape[0], _p(target),
                           float(max_correspondence_distance), _p(init_t), int(max_iteration),
                           float(relative_fitness), float(relative_rmse), _p(out_T), _p(stats))
    if rc != 1:
        raise RuntimeError("genpc_icp_batch failed (rc=%d): %s" % (rc, _lib.last_error()))
    host = buf.cpu().numpy()
    T = host[:k * 16].reshape(k, 4, 4)
    st = host[k * 16:].reshape(k, 3)
    if np.asarray(init).ndim == 2:
        return T[0], float(st[0, 0]), float(st[0, 1]), int(st[0, 2])
    return T, st[:, 0], st[:, 1], st[:, 2].astype(int)


def icp_with_scaling_xyz(source, target, scales, max_correspondence_distance=0.05, init_transform=None):
    """reg_xyz.py:9-21: the source is scaled per axis first (the reference does it in
    place on the open3d cloud), then ICP.  Returns (transformation, scaled_source)."""
    s = torch.as_tensor(np.asarray(scales, np.float64), device=source.device)
    scaled = (source.double() * s).float()
    T, _, _, _ = registration_icp(scaled, target, max_correspondence_distance,
                                  np.eye(4) if init_transform is None else init_transform)
    return T, scaled


def _scaled_inits(T1, scales):
    """[K,4,4]: T1 @ diag(scale, scale, scale, 1) for every scale (reg_xyz.py:31-36)."""
    inits = []
    for sc in scales:
        S = np.eye(4)
        S[:3, :3] *= sc
        inits.append(T1 @ S)
    return np.stack(inits)


def icp_with_scaling(source, target, scale, max_correspondence_distance=0.05, init_transform=None):
    """reg_xyz.py:24-38: ICP, then ICP again from result @ diag(scale).  `scale` may be
    a sequence: the first ICP is shared and the second runs as one batch."""
    init = np.eye(4) if init_transform is None else np.asarray(init_transform, np.float64)
    T1, _, _, _ = registration_icp(source, target, max_correspondence_distance, init)
    scales = np.atleast_1d(np.asarray(scale, np.float64))
    T2, fit, rmse, its = registration_icp(source, target, max_correspondence_distance, _scaled_inits(T1, scales))
    if np.ndim(scale) == 0:
        return T2[0]
    return T2


def _partial_cd_scores(src_b, tgt_b, cd_inv_weight):
    """chamfer_partial_l1(src, tgt) + w * chamfer_partial_l1(tgt, src) per batch row."""
    d1, d2, _, _ = chamfer_3DDist()(src_b, tgt_b)
    return torch.sqrt(d1).mean(1) + torch.sqrt(d2).mean(1) * cd_inv_weight


def coarse_scale_sweep(source_down, target_down, cd_inv_weight=0.5, scales=None, max_correspondence_distance=0.075):
    """The 11-scale sweep of reg() (reg_xyz.py:146-173).  Returns (best_scale, best_loss,
    coarse_transformation) with the reference's strict '<' (first minimum wins)."""
    if scales is None:
        scales = np.linspace(1.5, 0.8, 11)
    T = icp_with_scaling(source_down, target_down, scales, max_correspondence_distance)      # [K,4,4]
    inv = torch.as_tensor(np.linalg.inv(T), device=source_down.device)                        # :161-162
    tgt = target_down.double()
    tgt_k = (tgt @ inv[:, :3, :3].transpose(1, 2) + inv[:, None, :3, 3]).float().contiguous()
    src_k = source_down.float()[None].expand(len(scales), -1, -1).contiguous()
    cd = _partial_cd_scores(src_k, tgt_k, cd_inv_weight).cpu().numpy()
    best = int(np.argmin(cd))             # np.argmin returns the first minimum == strict '<' update
    return float(scales[best]), float(cd[best]), T[best]


def _scale_candidates(ranges, steps):
    """[steps^3,3] float64 (x, y, z) scales of the fine search, in the order z (outer), x, y (inner) (reg_xyz.py:66-75)."""
    xs = np.linspace(ranges[0][0], ranges[0][1], steps)
    ys = np.linspace(ranges[1][0], ranges[1][1], steps)
    zs = np.linspace(ranges[2][0], ranges[2][1], steps)
    gz, gx, gy = np.meshgrid(zs, xs, ys, indexing="ij")
    return np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1).astype(np.float64)


def iterative_scale_search(source_pcd, target_pcd, scale_ranges, scale_steps, init_transform=None, cd_inv_weight=0):
    """reg_xyz.py:60-96.  Returns (best_scales_transformation [4,4], best_loss,
    best_transformation [4,4]).  Candidate order z (outer), x, y (inner), strict '<'."""
    source = source_pcd.contiguous().float()
    target = target_pcd.contiguous().float()
    _lib.check_tensors((("source", source), ("target", target)))
    cand = _scale_candidates(scale_ranges, scale_steps)
    scales_t = torch.from_numpy(cand.astype(np.float32)).to(source.device)
    scores = torch.empty(len(cand), device=source.device)
    rc = _lib.on_device_of(source, _L.genpc_scale_search_scores, len(cand), source.shape[0], _p(source),
                           target.shape[0], _p(target), _p(scales_t), float(cd_inv_weight), _p(scores))
    if rc != 1:
        raise RuntimeError("genpc_scale_search_scores failed (rc=%d): %s" % (rc, _lib.last_error()))
    sc = scores.cpu().numpy()
    best = int(np.argmin(sc))
    best_scales = cand[best]
    best_T, _ = icp_with_scaling_xyz(source, target, best_scales, max_correspondence_distance=0.075,
                                     init_transform=np.eye(4) if init_transform is None else init_transform)
    S = np.eye(4)
    S[0, 0], S[1, 1], S[2, 2] = best_scales
    return S, float(sc[best]), best_T


# ---------------------------------------------------------------------------
# reg(): the composition of the stages above (reg_xyz.py:99-205) on tensors.
# ---------------------------------------------------------------------------
def get_rotate_matrix(axis, angle):
    """utils/dataUtils.py:455-472 (degrees)."""
    a = angle * np.pi / 180
    c, s = np.cos(a), np.sin(a)
    if axis == "x":
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    if axis == "y":
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    if axis == "z":
        return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    raise ValueError("axis should be x,y,z")


def normalize_numpy(xyz, range=1.0):
    """utils/dataUtils.py:561-581 on a tensor: bbox-centre, divide by the largest
    extent, scale to [-range, range].  Returns (normalised, centre, scale_factor)."""
    vmin, vmax = xyz.min(0).values, xyz.max(0).values
    center = (vmax + vmin) / 2.0
    scale_factor = (vmax - vmin).max()
    return (xyz - center) / scale_factor * (range / 0.5), center, scale_factor


def voxel_down_sample(xyz, voxel_size, colors=None):
    """Counterpart of open3d's PointCloud.voxel_down_sample (reg_xyz.py:154-155; open3d
    absent and unpinned): grid anchored at min_bound - voxel/2, one output point per
    occupied voxel = mean of its points (double, point order); `colors` [N,3], when given, are
    averaged per voxel the same way and returned as a second tensor.  Output order: ascending
    voxel index (open3d's is its hash-map order).  One call into the HIP library
    (csrc/voxel.hip: keys, radix sort, segmented mean).  voxel_size goes down as a double."""
    pts = xyz.contiguous().float()
    _lib.check_tensors((("xyz", pts),))
    n = pts.shape[0]
    col = None
    if colors is not None:
        col = colors.contiguous().float()
        _lib.check_tensors((("colors", col),))
        if col.shape != pts.shape:
            raise ValueError("voxel_down_sample: colors must be [N,3] like xyz")
    out = torch.empty(n, 3, device=pts.device)
    outc = torch.empty(n, 3, device=pts.device) if col is not None else None
    cnt = torch.empty(1, device=pts.device, dtype=torch.int32)
    rc = _lib.on_device_of(pts, _L.genpc_voxel_down_sample, n, _p(pts), _p(col), float(voxel_size), _p(out), _p(outc), _p(cnt))
    if rc == -1:
        raise ValueError("voxel_down_sample: voxel_size must be positive")
    if rc != 1:
        raise RuntimeError("genpc_voxel_down_sample failed: " + _lib.last_error())
    k = int(cnt.item())
    if k < 0:
        raise ValueError("voxel_down_sample: non-finite coordinate, or more than 2^21 voxels along an axis")
    if col is None:
        return out[:k].to(xyz.dtype)
    return out[:k].to(xyz.dtype), outc[:k].to(colors.dtype)


def _apply(T, xyz):
    """open3d PointCloud.transform: p <- T[:3,:3] p + T[:3,3] (double, like open3d)."""
    Tt = torch.as_tensor(np.asarray(T, np.float64), device=xyz.device)
    return (xyz.double() @ Tt[:3, :3].T + Tt[:3, 3]).to(xyz.dtype)


def _is_cfg(x):
    return hasattr(x, "output_path") and not torch.is_tensor(x)


def _check_file_form_options(who, takes, seed, kwargs):
    """The keyword checks of the file forms (`who`: the call as its messages spell it, `takes`: how they introduce its options)."""
    unknown = set(kwargs) - {"cd_only_pose", "rng"}
    if unknown:          # (the file form reads these options; anything else -- a misspelt one -- used to be dropped silently: ADVICE r3)
        raise TypeError("%s: unexpected keyword argument(s) %s (%s takes cd_only_pose, rng, seed)" % (who, sorted(unknown), takes))
    if seed is not None:
        if kwargs.get("rng") is not None:
            raise TypeError("%s: seed (the device sampler) and rng (the host sampler) exclude each other" % who)
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
            raise TypeError("%s: seed must be an int or None, got %r" % (who, seed))


def reg(cfg, flag, cd_inv_weight=0.5, diff_init=True, reg_fine_xyz=False, seed=None, **kwargs):
    """reg_xyz.py:99-223, same signature.

    (Deviation, file form: the PLY's double coordinates are cast to float32 before the voxel grids hash them; open3d
    hashes the doubles, so a point within float32 rounding of a voxel face can land in the neighbouring voxel.)
    File form (the reference's): ``reg(cfg, flag, cd_inv_weight, diff_init, reg_fine_xyz)`` reads
    ``{cfg.output_path}/{flag}/color_point.ply`` (the partial cloud with the colours colorPoint gave
    it) and ``{flag}_{cfg.generative_model}.glb`` (the generated mesh; 163 840 surface samples with
    their colours), aligns them and writes ``{flag}_fused.ply`` WITH COLOURS (:207-219); returns the
    dict of `reg_tensors` plus ``fused`` / ``fused_col`` / ``fused_path``.  Raises FileNotFoundError
    like the reference when an input is missing.  ``seed`` (an int; file form only): both samplings of the mesh -- these
    163 840 and the pose initialisation's 120 000 -- are drawn on the device by ``glb2point_gpu`` and are reproducible from
    it; with ``seed=None`` the host sampler runs as before (``rng=`` included).  ``seed`` together with ``rng`` raises.
    Tensor form: ``reg(partial_xyz, complete_xyz, ...)`` = `reg_tensors` (no files)."""
    if not _is_cfg(cfg):
        if seed is not None:
            raise TypeError("reg(partial_xyz, complete_xyz, ...): seed belongs to the file form (the tensor form samples nothing)")
        return reg_tensors(cfg, flag, cd_inv_weight=cd_inv_weight, diff_init=diff_init, reg_fine_xyz=reg_fine_xyz, **kwargs)
    import os
    from .optim_registration.diff_obj_pose import object_pose_optimization
    from .utils.dataUtils import read_ply, save_ply_xyzrgb
    from .utils.mesh_io import glb2point, glb2point_gpu
    _check_file_form_options("reg(cfg, flag, ...)", "the file form", seed, kwargs)
    path = cfg.output_path
    ply = f"{path}/{flag}/color_point.ply"
    glb = f"{path}/{flag}/{flag}_{cfg.generative_model}.glb"
    for f in (ply, glb):                                                # :103-108
        if not os.path.exists(f):
            print(f"Path {f} does not exist.")
            raise FileNotFoundError(f"Path {f} does not exist.")
    dev = torch.device(getattr(cfg, "device", "cuda"))
    diff_transform = None
    if diff_init:                                                       # :109-122
        diff_transform = np.linalg.inv(object_pose_optimization(
            glb_path=glb, point_path=ply, radius=0.02, lr=0.01, iters=200, render_size=224, vis=True, device=dev,
            cd_only=kwargs.get("cd_only_pose", False), seed=seed).astype(np.float64))
    sxyz, scol = read_ply(ply)                                          # :124 o3d.io.read_point_cloud
    if seed is None:
        txyz, tcol = glb2point(glb, num_points=163840, rng=kwargs.get("rng"))                  # :125
    else:
        txyz, tcol = glb2point_gpu(glb, num_points=163840, seed=seed, device=dev)              # (device tensors: no upload below)
    if scol is None:
        scol = np.zeros_like(sxyz)                                      # an open3d cloud without colours: fused file stays valid
    out = reg_tensors(torch.as_tensor(sxyz, dtype=torch.float32, device=dev), torch.as_tensor(txyz, dtype=torch.float32, device=dev),
                      generative_model=cfg.generative_model, dataset=getattr(cfg, "dataset", "redwood"),
                      cd_inv_weight=cd_inv_weight, diff_init=diff_init, reg_fine_xyz=reg_fine_xyz,
                      partial_col=torch.as_tensor(scol, dtype=torch.float32, device=dev),
                      complete_col=torch.as_tensor(tcol, dtype=torch.float32, device=dev), diff_transform=diff_transform)
    fused, fused_col = fuse(out["source"], out["target"], num_points=20000, distance_threshold=0.0001, std_ratio=2.5,
                            source_col=out["source_col"], target_col=out["target_col"])       # :207-217
    out.update(fused=fused, fused_col=fused_col, fused_path=f"{path}/{flag}/{flag}_fused.ply")
    save_ply_xyzrgb(fused.double().cpu().numpy(), fused_col.double().cpu().numpy(), out["fused_path"])     # :221
    return out


def reg_tensors(partial_xyz, complete_xyz, generative_model="trellis", dataset="redwood", cd_inv_weight=0.5,
                diff_init=True, reg_fine_xyz=False, pose_voxel=0.02, cd_only_pose=False, partial_col=None,
                complete_col=None, diff_transform=None):
    """reg_xyz.py:99-205 on tensors, without file I/O and without the fusion tail.
    partial_xyz: the observed cloud (color_point.ply), complete_xyz: points sampled from
    the generated mesh (glb2point); partial_col / complete_col: their colours ([N,3] in [0,1], None =
    white in the pose loss) -- they feed the silhouette term of the pose initialisation and are carried
    to the outputs.  diff_transform: a precomputed inverse pose (the file form computes it from its own
    120 000-point sampling like the reference); None runs object_pose_optimization on both clouds
    voxel-down-sampled at `pose_voxel` (load_point_cloud's radius).  Returns a dict with the aligned
    clouds (`source`, `target`: both back in the partial cloud's original frame, as at :200-205;
    `source_col`, `target_col`) and every intermediate transform."""
    from .optim_registration.diff_obj_pose import object_pose_optimization
    source = partial_xyz.contiguous().float()
    target = complete_xyz.contiguous().float()
    scol = None if partial_col is None else partial_col.contiguous().float()
    tcol = None if complete_col is None else complete_col.contiguous().float()
    out = {}
    if not diff_init:
        diff_transform = np.eye(4)
    elif diff_transform is None:                                        # :109-122
        if tcol is not None:
            tv, tvc = voxel_down_sample(target, pose_voxel, colors=tcol)
        else:
            tv, tvc = voxel_down_sample(target, pose_voxel), None
        if scol is not None:
            sv, svc = voxel_down_sample(source, pose_voxel, colors=scol)
        else:
            sv, svc = voxel_down_sample(source, pose_voxel), None
        T = object_pose_optimization(tv, sv, radius=0.02, lr=0.01, iters=200, render_size=224, cd_only=cd_only_pose,
                                     complete_col=tvc, partial_col=svc)
        diff_transform = np.linalg.inv(T.astype(np.float64))
    out["diff_transform"] = diff_transform
    source = _apply(diff_transform, source)                             # :126
    target, _, _ = normalize_numpy(target, range=0.5)                   # :130
    if generative_model in ("instantmesh",):                            # :132-137
        source, keep = remove_noise_from_point_cloud(source)
        if scol is not None:
            scol = scol[keep]
        target = (target.double() @ torch.as_tensor(get_rotate_matrix("x", 90).T, device=target.device)
                  @ torch.as_tensor(get_rotate_matrix("y", 90).T, device=target.device)).float()
    best_scale, best_loss, coarse = coarse_scale_sweep(voxel_down_sample(source, 0.03), voxel_down_sample(target, 0.03),
                                                       cd_inv_weight=cd_inv_weight)            # :146-173
    out.update(best_scale=best_scale, coarse_loss=best_loss, coarse_transformation=coarse)
    if reg_fine_xyz:                                                    # :176-199
        source = _apply(coarse, source)
        tv = 0.04 if dataset in ("pcn", "kitti") else 0.03
        src_s = source if dataset in ("pcn", "kitti") else voxel_down_sample(source, 0.03)
        S, loss_xyz, T_xyz = iterative_scale_search(src_s, voxel_down_sample(target, tv), [(0.8, 1.2)] * 3, 10,
                                                    init_transform=np.eye(4), cd_inv_weight=cd_inv_weight)
        out.update(best_scales_transformation=S, xyz_loss=loss_xyz, best_transformation_xyz=T_xyz)
        target = _apply(np.linalg.inv(S), target)
        target = _apply(np.linalg.inv(T_xyz), target)
        source = _apply(np.linalg.inv(coarse), source)
    target = _apply(np.linalg.inv(coarse), target)                      # :201-205
    target = _apply(np.linalg.inv(diff_transform), target)
    source = _apply(np.linalg.inv(diff_transform), source)
    out.update(source=source, target=target, source_col=scol, target_col=tcol)
    return out


# ---------------------------------------------------------------------------
# Fusion tail of reg() (reg_xyz.py:207-219), SURVEY 8f row f2.
# ---------------------------------------------------------------------------
def remove_close_points(source_xyz, target_xyz, distance_threshold=0.0001):
    """reg_xyz.py:41-57: drop every target point whose nearest source point is closer
    than sqrt(distance_threshold) (open3d's KD-tree returns SQUARED distances, so the
    reference's 1e-4 is 0.01 units).  One NN launch instead of a Python loop of KD-tree
    queries (measured at 163840 x 16384: 147 us on the default MFMA filter; the radius-limited
    cell search, chamfer_3D.nm_distance_within, gives the same mask in 156 us -- no gain yet).
    Returns (filtered target [K,3], keep mask [M]) -- index colours with the mask (:56)."""
    from . import chamfer_3D
    src = source_xyz.contiguous().float()
    tgt = target_xyz.contiguous().float()
    d = torch.empty(1, tgt.shape[0], device=tgt.device)
    i = torch.empty(1, tgt.shape[0], device=tgt.device, dtype=torch.int32)
    if tgt.shape[0] == 0 or src.shape[0] == 0:
        return tgt, torch.ones(tgt.shape[0], dtype=torch.bool, device=tgt.device)
    if chamfer_3D.nm_distance(tgt[None], src[None], d, i) != 1:
        raise RuntimeError("nm_distance failed: " + _lib.last_error())
    keep = ~(d[0] < distance_threshold)
    return tgt[keep], keep


def fuse(source_xyz, target_xyz, num_points=20000, distance_threshold=0.0001, std_ratio=2.5, source_col=None,
         target_col=None, side_fps=None):
    """reg_xyz.py:207-217: partial + (complete minus what the partial already covers),
    farthest-point-sampled to `num_points`, then the statistical outlier filter
    (std_ratio 2.5 as at :217; None skips it).  With source_col / target_col the colours follow their
    points through all three steps (:56,:212-216) and (fused, fused_col) is returned.
    side_fps: [(cloud [N,3], k), ...] -- independent subsamplings the caller needs anyway (the metric's
    ground-truth cloud, main.py:21) ride along in the fused cloud's FPS launch (a pass costs its longest
    chain of sequential steps, not the sum); their index tensors are appended to the return value."""
    from .fps import fps_sampling, fps_sampling_multi
    with_col = source_col is not None and target_col is not None
    filtered, keep = remove_close_points(source_xyz, target_xyz, distance_threshold)
    fused = torch.cat([source_xyz.float(), filtered], dim=0).contiguous()
    col = torch.cat([source_col.float(), target_col.float()[keep]], dim=0) if with_col else None
    side = []
    if side_fps:
        need = fused.shape[0] > num_points
        clouds = ([fused] if need else []) + [c.contiguous().float() for c, _ in side_fps]
        ks = ([num_points] if need else []) + [k for _, k in side_fps]
        got = fps_sampling_multi(clouds, ks)
        if need:
            idx = got[0].long()
            fused = fused[idx]
            col = col[idx] if with_col else None
        side = got[1:] if need else got
    elif fused.shape[0] > num_points:
        idx = fps_sampling(fused, num_points).long()
        fused = fused[idx]
        col = col[idx] if with_col else None
    if std_ratio is not None:                                            # :217
        fused, ok = remove_noise_from_point_cloud(fused, std_ratio=std_ratio)
        col = col[ok] if with_col else None
    out = (fused, col) if with_col else fused
    if side_fps:
        return out, side
    return out


def knn_mean_distance(xyz, k=20):
    """Mean distance of every point to its k nearest points of the same cloud (the
    point itself included) -- the statistic of open3d's remove_statistical_outlier."""
    pts = xyz.contiguous().float()
    _lib.check_tensors((("xyz", pts),))
    out = torch.empty(pts.shape[0], device=pts.device)
    rc = _lib.on_device_of(pts, _L.genpc_knn_mean_distance, pts.shape[0], _p(pts), int(k), _p(out))
    if rc == -1:
        raise ValueError("knn_mean_distance: k must be 8, 16, 20 or 32")
    if rc != 1:
        raise RuntimeError("genpc_knn_mean_distance failed: " + _lib.last_error())
    return out


def remove_noise_from_point_cloud(xyz, nb_neighbors=20, std_ratio=1.5):
    """utils/dataUtils.py:648-662 (open3d remove_statistical_outlier) on a tensor: keeps
    points whose mean k-NN distance is below mean + std_ratio * std (sample std, double).
    Returns (filtered [K,3], keep mask [N])."""
    m = knn_mean_distance(xyz, nb_neighbors).double()
    mean = m.mean()
    std = torch.sqrt(((m - mean) ** 2).sum() / (m.numel() - 1))
    keep = m < mean + std_ratio * std
    return xyz[keep], keep


# ---------------------------------------------------------------------------
# The ragged forms: S clouds of any sizes per library call (the batched scan pipeline's fusion tail).
# ---------------------------------------------------------------------------
OUTLIER_RAGGED_MAX_CLOUDS = 384          # include/genpc_hip.h: clouds per genpc_knn_mean_distance_ragged / genpc_outlier_filter_ragged call


def knn_mean_distance_ragged(clouds, k=20):
    """``knn_mean_distance`` for S clouds of any sizes: a list of [N_j,3] float32 GPU tensors, or packed as (points [T,3],
    offsets) with S + 1 host ints.  Returns a list of float32 [N_j] tensors, views of one packed result; cloud j's are the
    bits of ``knn_mean_distance(clouds[j], k)``.  One library call per 384 clouds (genpc_knn_mean_distance_ragged: two
    launches each), nothing waits for the result.  An empty cloud gives an empty tensor."""
    pts, off = ragged_side(clouds, "knn_mean_distance_ragged")
    if int(k) not in (8, 16, 20, 32):
        raise ValueError("knn_mean_distance_ragged: k must be 8, 16, 20 or 32")
    if len(off) == 1:
        return []
    _lib.require_gpu(pts)
    out = torch.empty(pts.shape[0], device=pts.device)
    for a, b, oa in chunks(OUTLIER_RAGGED_MAX_CLOUDS, off):
        rc = _lib.on_device_of(pts, _L.genpc_knn_mean_distance_ragged, b - a, host_ints(oa)[1], _p(pts[off[a]:off[b]]), int(k), _p(out[off[a]:off[b]]))
        if rc != 1:
            raise RuntimeError("genpc_knn_mean_distance_ragged failed (%d): %s" % (rc, _lib.last_error()))
    return [out[off[j]:off[j + 1]] for j in range(len(off) - 1)]


def _outlier_filter_ragged(pts, off, nb_neighbors, std_ratio):
    """keep (bool [T], packed), stats (float64 [S,3]: mean, std, threshold), kept (int32 [S]) of the packed clouds."""
    s = len(off) - 1
    keep = torch.empty(pts.shape[0], dtype=torch.uint8, device=pts.device)
    # (a library call without a point enqueues nothing: its clouds are empty, and these are an empty cloud's words)
    stats = torch.full((s, 3), float("nan"), dtype=torch.float64, device=pts.device)
    kept = torch.zeros(s, dtype=torch.int32, device=pts.device)
    for a, b, oa in chunks(OUTLIER_RAGGED_MAX_CLOUDS, off):
        rc = _lib.on_device_of(pts, _L.genpc_outlier_filter_ragged, b - a, host_ints(oa)[1], _p(pts[off[a]:off[b]]), int(nb_neighbors),
                               float(std_ratio), None, _p(stats[a:b]), _p(keep[off[a]:off[b]]), _p(kept[a:b]))
        if rc != 1:
            raise RuntimeError("genpc_outlier_filter_ragged failed (%d): %s" % (rc, _lib.last_error()))
    return keep.view(torch.bool), stats, kept


def remove_noise_from_point_clouds(clouds, nb_neighbors=20, std_ratio=1.5, return_stats=False):
    """``remove_noise_from_point_cloud`` for S clouds of any sizes (a list of [N_j,3] float32 GPU tensors, or packed as
    (points, offsets)): returns (filtered: list of [K_j,3], keep: list of bool [N_j]); with return_stats also float64 [S,3]
    = (mean, std, threshold) per cloud and int32 [S] = K_j, both on the device.  One library call per 384 clouds
    (genpc_outlier_filter_ragged): means, statistics and mask are made on the device, the sums in the order
    include/genpc_hip.h defines -- not torch's, so a point whose mean lies within rounding of the threshold (a relative 1e-15)
    may fall on the other side than ``remove_noise_from_point_cloud`` puts it.  The host waits for the K_j, which size the
    filtered tensors, and in the boolean index over the packed points: twice, whatever S is."""
    pts, off = ragged_side(clouds, "remove_noise_from_point_clouds")
    if int(nb_neighbors) not in (8, 16, 20, 32):
        raise ValueError("remove_noise_from_point_clouds: nb_neighbors must be 8, 16, 20 or 32")
    s = len(off) - 1
    if s == 0 and not pts.is_cuda:             # (an empty list has no device: the current one)
        pts = pts.to(torch.device("cuda", torch.cuda.current_device()))
    _lib.require_gpu(pts)
    keep, stats, kept = _outlier_filter_ragged(pts, off, nb_neighbors, std_ratio)
    sizes = kept.tolist()
    filtered = list(torch.split(pts[keep], sizes)) if s else []
    keeps = [keep[off[j]:off[j + 1]] for j in range(s)]
    if return_stats:
        return filtered, keeps, stats, kept
    return filtered, keeps


def fuse_scans(sources, targets, num_points=20000, distance_threshold=0.0001, std_ratio=2.5, source_cols=None, target_cols=None):
    """``fuse`` for S scans at once: sources / targets are lists of [N_j,3] / [M_j,3] float32 GPU tensors or packed
    (points, offsets); source_cols / target_cols, when both are given, lists of their colours.  One ``nm_distance_ragged``
    call makes all the ``remove_close_points`` masks, one ``fps_sampling_multi`` samples the scans that exceed num_points,
    one ``remove_noise_from_point_clouds`` filters them all (std_ratio None skips it).  Returns a list of fused clouds, or of
    (fused, col) pairs; scan j's is what ``fuse(sources[j], targets[j], ...)`` returns, up to the caveat of
    ``remove_noise_from_point_clouds``."""
    from .fps import fps_sampling_multi
    from .loss_functions.Chamfer3D.dist_chamfer_ragged import _one_way
    sp, soff = ragged_side(sources, "fuse_scans", "sources")
    tp, toff = ragged_side(targets, "fuse_scans", "targets")
    if len(soff) != len(toff):
        raise ValueError("fuse_scans: %d sources against %d targets" % (len(soff) - 1, len(toff) - 1))
    s = len(soff) - 1
    with_col = source_cols is not None and target_cols is not None
    if with_col and (len(source_cols) != s or len(target_cols) != s):
        raise ValueError("fuse_scans: one colour tensor per cloud (%d scans, %d source_cols, %d target_cols)" % (s, len(source_cols), len(target_cols)))
    if s == 0:
        return []
    _lib.require_gpu(sp, tp)
    if sp.device != tp.device:
        raise ValueError("fuse_scans: sources and targets are on different devices")
    if with_col:
        for name, cols, off in (("source_cols", source_cols, soff), ("target_cols", target_cols, toff)):
            for j, c in enumerate(cols):
                if not torch.is_tensor(c) or tuple(c.shape) != (off[j + 1] - off[j], 3):
                    raise ValueError("fuse_scans: %s[%d] must be [%d,3] like its cloud" % (name, j, off[j + 1] - off[j]))
    # remove_close_points for every scan: the targets ask, the sources answer.  A scan with an empty side keeps its targets.
    live = [j for j in range(s) if soff[j + 1] > soff[j] and toff[j + 1] > toff[j]]
    keep_t = torch.ones(tp.shape[0], dtype=torch.bool, device=tp.device)
    if len(live) == s:
        d, _ = _one_way(tp, toff, sp, soff)
        keep_t = ~(d < distance_threshold)
    elif live:
        q, qoff = ragged_side([tp[toff[j]:toff[j + 1]] for j in live], "fuse_scans", "targets")
        t, t_off = ragged_side([sp[soff[j]:soff[j + 1]] for j in live], "fuse_scans", "sources")
        d, _ = _one_way(q, qoff, t, t_off)
        for i, j in enumerate(live):
            keep_t[toff[j]:toff[j + 1]] = ~(d[qoff[i]:qoff[i + 1]] < distance_threshold)
    bounds = torch.tensor(toff, device=tp.device)
    csum = torch.cat([keep_t.new_zeros(1, dtype=torch.int64), torch.cumsum(keep_t, 0)])
    sizes = (csum[bounds[1:]] - csum[bounds[:-1]]).tolist()                  # (the one host read of this step)
    filtered = torch.split(tp[keep_t], sizes)
    fused = [torch.cat([sp[soff[j]:soff[j + 1]], filtered[j]], dim=0) for j in range(s)]
    cols = None
    if with_col:
        cols = [torch.cat([source_cols[j].float(), target_cols[j].float()[keep_t[toff[j]:toff[j + 1]]]], dim=0) for j in range(s)]
    big = [j for j in range(s) if fused[j].shape[0] > num_points]
    if big:
        for j, idx in zip(big, fps_sampling_multi([fused[j] for j in big], [num_points] * len(big))):
            idx = idx.long()
            fused[j] = fused[j][idx]
            if with_col:
                cols[j] = cols[j][idx]
    if std_ratio is not None:
        fused, oks = remove_noise_from_point_clouds(fused, std_ratio=std_ratio)
        if with_col:
            cols = [cols[j][oks[j]] for j in range(s)]
    return [(fused[j], cols[j]) for j in range(s)] if with_col else list(fused)


# ---------------------------------------------------------------------------
# The stage between the pose initialisation and the fusion tail, for S scans per library call: the voxel grids and the
# coarse ICP sweep of reg() (reg_xyz.py:146-173).
# ---------------------------------------------------------------------------
VOXEL_RAGGED_MAX_CLOUDS = 256            # include/genpc_hip.h: GENPC_VOXEL_RAGGED_MAX_CLOUDS
ICP_RAGGED_MAX_PAIRS = 256               # include/genpc_hip.h: GENPC_ICP_RAGGED_MAX_PAIRS


def voxel_down_sample_clouds(clouds, voxel_size, colors=None):
    """``voxel_down_sample`` for S clouds of any sizes: a list of [N_j,3] float32 GPU tensors, or packed as (points [T,3],
    offsets) with S + 1 host ints.  voxel_size: one float for all, or one per cloud (reg mixes 0.02, 0.03 and 0.04); colors,
    when given, are packed or listed like the clouds.  Returns a list of [K_j,3] tensors -- with colours (list, list) -- each a
    view of one packed result; cloud j's are the bits of ``voxel_down_sample(clouds[j], voxel_size[j])``.  One library call per
    256 clouds (genpc_voxel_down_sample_ragged: a fixed number of launches) and ONE read-back, of all the counts, whatever S
    is.  A cloud with a non-finite coordinate or more than 2^21 voxels along an axis raises ValueError naming it."""
    import ctypes
    fn = "voxel_down_sample_clouds"
    pts, off = ragged_side(clouds, fn)
    s = len(off) - 1
    sizes = [float(voxel_size)] * s if np.ndim(voxel_size) == 0 else [float(v) for v in voxel_size]
    if len(sizes) != s:
        raise ValueError("%s: %d voxel sizes for %d clouds" % (fn, len(sizes), s))
    for j, v in enumerate(sizes):
        if not v > 0:
            raise ValueError("%s: the voxel size of cloud %d must be positive" % (fn, j))
    col = None
    if colors is not None:
        col, coff = ragged_side(colors, fn, "colors")
        if coff != off:
            raise ValueError("%s: colors must be [N_j,3] like their clouds" % fn)
    if s == 0:
        return [] if col is None else ([], [])
    _lib.require_gpu(pts)
    if col is not None:
        _lib.require_gpu(col)
        if col.device != pts.device:
            raise ValueError("%s: clouds and colors are on different devices" % fn)
    out = torch.empty_like(pts)
    outc = torch.empty_like(col) if col is not None else None
    counts = torch.empty(s, dtype=torch.int32, device=pts.device)
    for a, b, oa in chunks(VOXEL_RAGGED_MAX_CLOUDS, off):
        vs = (ctypes.c_double * (b - a))(*sizes[a:b])
        rc = _lib.on_device_of(pts, _L.genpc_voxel_down_sample_ragged, b - a, host_ints(oa)[1], _p(pts[off[a]:off[b]]),
                               _p(None if col is None else col[off[a]:off[b]]), ctypes.cast(vs, ctypes.c_void_p), _p(out[off[a]:off[b]]),
                               _p(None if outc is None else outc[off[a]:off[b]]), _p(counts[a:b]))
        if rc != 1:
            raise RuntimeError("genpc_voxel_down_sample_ragged failed (%d): %s" % (rc, _lib.last_error()))
    got = counts.tolist()                     # (the one host read)
    for j, k in enumerate(got):
        if k < 0:
            raise ValueError("%s: cloud %d has a non-finite coordinate, or more than 2^21 voxels along an axis" % (fn, j))
    down = [out[off[j]:off[j] + got[j]] for j in range(s)]
    if col is None:
        return down
    return down, [outc[off[j]:off[j] + got[j]] for j in range(s)]


def registration_icp_ragged(sources, targets, max_correspondence_distance, inits, max_iteration=30, relative_fitness=1e-6,
                            relative_rmse=1e-6):
    """``registration_icp`` for S (source, target) pairs of any sizes at once: sources / targets are lists of [N_j,3] / [M_j,3]
    float32 GPU tensors or packed (points, offsets); inits a list of S arrays, [K_j,4,4] or [4,4] float64 (K_j = 0 skips the
    pair).  Returns a list of (transformation [K_j,4,4] float64 numpy, fitness [K_j], inlier_rmse [K_j], iters [K_j]) -- a
    [4,4] init gives unbatched values, as registration_icp does.  One library call per 256 pairs (genpc_icp_batch_ragged: the
    pairs whose target fits the one-workgroup solve share ONE launch and get the bits of registration_icp on the pair alone)
    and one copy back per call of this function."""
    fn = "registration_icp_ragged"
    sp, soff = ragged_side(sources, fn, "sources")
    tp, toff = ragged_side(targets, fn, "targets")
    if len(soff) != len(toff):
        raise ValueError("%s: %d sources against %d targets" % (fn, len(soff) - 1, len(toff) - 1))
    s = len(soff) - 1
    if not isinstance(inits, (list, tuple)) or len(inits) != s:
        raise ValueError("%s: inits is a list of one [K,4,4] or [4,4] array per pair (%d pairs)" % (fn, s))
    arrs, koff = [], [0]
    for j, init in enumerate(inits):
        a = np.asarray(init.detach().cpu() if torch.is_tensor(init) else init, np.float64)
        if a.shape != (4, 4) and (a.ndim != 3 or a.shape[1:] != (4, 4)):
            raise ValueError("%s: inits[%d] must be [K,4,4] or [4,4], got %s" % (fn, j, a.shape))
        arrs.append(a.reshape(-1, 4, 4))
        koff.append(koff[-1] + arrs[-1].shape[0])
        if arrs[-1].shape[0] and (soff[j + 1] == soff[j] or toff[j + 1] == toff[j]):
            raise ValueError("%s: pair %d has candidates and an empty %s" % (fn, j, "source" if soff[j + 1] == soff[j] else "target"))
    if s == 0:
        return []
    _lib.require_gpu(sp, tp)
    if sp.device != tp.device:
        raise ValueError("%s: sources and targets are on different devices" % fn)
    k = koff[-1]
    dev = sp.device
    init_t = torch.as_tensor(np.concatenate(arrs, axis=0).reshape(k, 16)).contiguous().to(dev)
    buf = torch.empty(k * 19, dtype=torch.float64, device=dev)           # transforms and statistics: one copy back
    out_T, stats = buf[:k * 16].view(k, 16), buf[k * 16:].view(k, 3)
    for a, b, sa, ta, ka in chunks(ICP_RAGGED_MAX_PAIRS, soff, toff, koff):
        rc = _lib.on_device_of(sp, _L.genpc_icp_batch_ragged, b - a, host_ints(sa)[1], host_ints(ta)[1], host_ints(ka)[1],
                               _p(sp[soff[a]:soff[b]]), _p(tp[toff[a]:toff[b]]),
                               float(max_correspondence_distance), _p(init_t[koff[a]:koff[b]]), int(max_iteration),
                               float(relative_fitness), float(relative_rmse), _p(out_T[koff[a]:koff[b]]), _p(stats[koff[a]:koff[b]]))
        if rc != 1:
            raise RuntimeError("genpc_icp_batch_ragged failed (rc=%d): %s" % (rc, _lib.last_error()))
    host = buf.cpu().numpy()
    T = host[:k * 16].reshape(k, 4, 4)
    st = host[k * 16:].reshape(k, 3)
    res = []
    for j in range(s):
        a, b = koff[j], koff[j + 1]
        if np.ndim(inits[j]) == 2:
            res.append((T[a], float(st[a, 0]), float(st[a, 1]), int(st[a, 2])))
        else:
            res.append((T[a:b], st[a:b, 0], st[a:b, 1], st[a:b, 2].astype(int)))
    return res


def coarse_scale_sweeps(sources_down, targets_down, cd_inv_weight=0.5, scales=None, max_correspondence_distance=0.075,
                        return_all=False):
    """``coarse_scale_sweep`` for S scans at once (lists of [N_j,3] / [M_j,3] float32 GPU tensors, or packed): returns a list of
    (best_scale, best_loss, coarse_transformation), with return_all also every candidate's transform [K,4,4] and score [K].
    Two ``registration_icp_ragged`` calls -- one candidate per scan from the identity, then len(scales) per scan from
    T1_j @ diag(scale) -- and the S * len(scales) (source, inverse-transformed target) pairs scored through ``chamfer_ragged``;
    the first minimum wins, as the reference's strict '<'.  The host reads back three times whatever S is."""
    from .loss_functions.Chamfer3D.dist_chamfer_ragged import chamfer_ragged
    fn = "coarse_scale_sweeps"
    sp, soff = ragged_side(sources_down, fn, "sources_down")
    tp, toff = ragged_side(targets_down, fn, "targets_down")
    if len(soff) != len(toff):
        raise ValueError("%s: %d sources against %d targets" % (fn, len(soff) - 1, len(toff) - 1))
    s = len(soff) - 1
    if s == 0:
        return []
    if scales is None:
        scales = np.linspace(1.5, 0.8, 11)
    scales = np.atleast_1d(np.asarray(scales, np.float64))
    k = len(scales)
    md = max_correspondence_distance
    first = registration_icp_ragged((sp, soff), (tp, toff), md, [np.eye(4)] * s)
    inits = [_scaled_inits(first[j][0], scales) for j in range(s)]          # icp_with_scaling: ICP again from result @ diag(scale)
    T = [r[0] for r in registration_icp_ragged((sp, soff), (tp, toff), md, inits)]          # S x [K,4,4]
    src_k, tgt_k, o1, o2 = [], [], [0], [0]
    for j in range(s):                                       # :161-162, per scan as coarse_scale_sweep writes it
        inv = torch.as_tensor(np.linalg.inv(T[j]), device=tp.device)
        tgt = tp[toff[j]:toff[j + 1]].double()
        tgt_k.append((tgt @ inv[:, :3, :3].transpose(1, 2) + inv[:, None, :3, 3]).float().reshape(-1, 3))
        src_k.append(sp[soff[j]:soff[j + 1]].repeat(k, 1))
        for _ in range(k):
            o1.append(o1[-1] + soff[j + 1] - soff[j])
            o2.append(o2[-1] + toff[j + 1] - toff[j])
    # (chamfer_ragged takes as many library calls as its pair limit asks for)
    d1, d2, _, _, _, _ = chamfer_ragged((torch.cat(src_k).contiguous(), o1), (torch.cat(tgt_k).contiguous(), o2))
    scores = []
    for j in range(s):
        a1, a2 = d1[o1[j * k]:o1[(j + 1) * k]].view(k, -1), d2[o2[j * k]:o2[(j + 1) * k]].view(k, -1)
        scores.append(torch.sqrt(a1).mean(1) + torch.sqrt(a2).mean(1) * cd_inv_weight)
    cd = torch.stack(scores).cpu().numpy()                   # [S,K]: one copy back
    out = []
    for j in range(s):
        best = int(np.argmin(cd[j]))                         # the first minimum == strict '<'
        r = (float(scales[best]), float(cd[j, best]), T[j][best])
        out.append(r + (T[j], cd[j].copy()) if return_all else r)
    return out


# ---------------------------------------------------------------------------
# The fine xyz scale search of reg() (reg_xyz.py:60-96, :176-199) for S scans per library call.
# ---------------------------------------------------------------------------
SCALE_SEARCH_RAGGED_MAX_PAIRS = 256      # include/genpc_hip.h: GENPC_SCALE_SEARCH_RAGGED_MAX_PAIRS


def _scale_search_scores_packed(sources, targets, scales, cd_inv_weight, fn):
    """(scores [K] float32 on the device -- None without a scan --, koff: S + 1 Python ints) of scale_search_scores_ragged."""
    sp, soff = ragged_side(sources, fn, "sources")
    tp, toff = ragged_side(targets, fn, "targets")
    if len(soff) != len(toff):
        raise ValueError("%s: %d sources against %d targets" % (fn, len(soff) - 1, len(toff) - 1))
    s = len(soff) - 1
    if not isinstance(scales, (list, tuple)) or len(scales) != s:
        raise ValueError("%s: scales is a list of one [K,3] array per pair (%d pairs)" % (fn, s))
    rows, koff = [], [0]
    for j, sc in enumerate(scales):
        a = sc.detach().float() if torch.is_tensor(sc) else torch.from_numpy(np.asarray(sc).astype(np.float32))
        if a.numel() == 0 and a.dim() == 1:
            a = a.reshape(0, 3)
        if a.dim() != 2 or a.shape[1] != 3:
            raise ValueError("%s: scales[%d] must be [K,3], got %s" % (fn, j, tuple(a.shape)))
        rows.append(a)
        koff.append(koff[-1] + a.shape[0])
        if a.shape[0] and (soff[j + 1] == soff[j] or toff[j + 1] == toff[j]):
            raise ValueError("%s: pair %d has candidates and an empty %s" % (fn, j, "source" if soff[j + 1] == soff[j] else "target"))
    if s == 0:
        return None, koff
    _lib.require_gpu(sp, tp)
    if sp.device != tp.device:
        raise ValueError("%s: sources and targets are on different devices" % fn)
    dev = sp.device
    if all(not r.is_cuda for r in rows):
        scales_t = torch.cat(rows).contiguous().to(dev)              # host candidates: one upload
    else:
        scales_t = torch.cat([r.to(dev) for r in rows]).contiguous()
    scores = torch.empty(koff[-1], device=dev)
    for a, b, sa, ta, ka in chunks(SCALE_SEARCH_RAGGED_MAX_PAIRS, soff, toff, koff):
        rc = _lib.on_device_of(sp, _L.genpc_scale_search_scores_ragged, b - a, host_ints(sa)[1], host_ints(ta)[1], host_ints(ka)[1],
                               _p(sp[soff[a]:soff[b]]), _p(tp[toff[a]:toff[b]]),
                               _p(scales_t[koff[a]:koff[b]]), float(cd_inv_weight), _p(scores[koff[a]:koff[b]]))
        if rc != 1:
            raise RuntimeError("genpc_scale_search_scores_ragged failed (rc=%d): %s" % (rc, _lib.last_error()))
    return scores, koff


def scale_search_scores_ragged(sources, targets, scales, cd_inv_weight=0):
    """The scores of ``iterative_scale_search`` for S (source, target) pairs of any sizes at once: sources / targets are lists of
    [N_j,3] / [M_j,3] float32 GPU tensors or packed (points, offsets); scales a list of S arrays or tensors [K_j,3] (K_j = 0
    skips the pair).  Returns a list of float32 [K_j] device tensors, views of one packed result: candidate k of pair j gets
    mean sqrt(NN(source_j * scales_j[k] -> target_j)) + cd_inv_weight * mean sqrt(NN(target_j -> source_j * scales_j[k])), the
    bits of genpc_scale_search_scores on the pair alone.  One library call per 256 pairs (genpc_scale_search_scores_ragged: two
    launches each, no copy of a cloud per candidate); nothing waits for the result."""
    scores, koff = _scale_search_scores_packed(sources, targets, scales, cd_inv_weight, "scale_search_scores_ragged")
    if scores is None:
        return []
    return [scores[koff[j]:koff[j + 1]] for j in range(len(koff) - 1)]


def iterative_scale_searches(sources, targets, scale_ranges, scale_steps, init_transforms=None, cd_inv_weight=0):
    """``iterative_scale_search`` for S scans at once (lists of [N_j,3] / [M_j,3] float32 GPU tensors, or packed): scale_ranges is
    three (lo, hi) pairs for all scans or a list of S such triples; init_transforms None or a list of S [4,4] arrays (None: the
    identity).  Returns a list of (best_scales_transformation [4,4], best_loss, best_transformation [4,4]); scan j's is what
    ``iterative_scale_search(sources[j], targets[j], ...)`` returns -- the scores and the winner bit for bit, the winner's ICP
    bit for bit where its target gets the one-workgroup ICP plan (``registration_icp_ragged``).  Candidate order z (outer), x,
    y (inner); the first minimum wins.  One ``scale_search_scores_ragged``, ONE read-back of all scores and one
    ``registration_icp_ragged`` over the winners, whatever S is.  A scan whose scores hold a NaN raises ValueError naming it."""
    fn = "iterative_scale_searches"
    sp, soff = ragged_side(sources, fn, "sources")
    tp, toff = ragged_side(targets, fn, "targets")
    if len(soff) != len(toff):
        raise ValueError("%s: %d sources against %d targets" % (fn, len(soff) - 1, len(toff) - 1))
    s = len(soff) - 1
    shape = np.shape(scale_ranges)
    if shape == (3, 2):
        ranges = [scale_ranges] * s
    elif shape == (s, 3, 2):
        ranges = list(scale_ranges)
    else:
        raise ValueError("%s: scale_ranges is three (lo, hi) pairs, or one such triple per scan (%d scans)" % (fn, s))
    if init_transforms is not None and (not isinstance(init_transforms, (list, tuple)) or len(init_transforms) != s):
        raise ValueError("%s: init_transforms is None or a list of one [4,4] array per scan (%d scans)" % (fn, s))
    inits = []
    for j in range(s):
        T = np.eye(4) if init_transforms is None or init_transforms[j] is None else np.asarray(init_transforms[j], np.float64)
        if T.shape != (4, 4):
            raise ValueError("%s: init_transforms[%d] must be [4,4], got %s" % (fn, j, T.shape))
        inits.append(T)
    cands = [_scale_candidates(r, scale_steps) for r in ranges]
    scores, koff = _scale_search_scores_packed((sp, soff), (tp, toff), cands, cd_inv_weight, fn)
    if s == 0:
        return []
    sc = scores.cpu().numpy()                                        # (the one read-back of the scores)
    best, scaled = [], []
    for j in range(s):
        sj = sc[koff[j]:koff[j + 1]]
        if np.isnan(sj).any():
            raise ValueError("%s: scan %d has a NaN score (a non-finite coordinate, or a scaled one that overflows)" % (fn, j))
        best.append(int(np.argmin(sj)))                              # the first minimum == strict '<'
        sv = torch.as_tensor(cands[j][best[j]], device=sp.device)
        scaled.append((sp[soff[j]:soff[j + 1]].double() * sv).float())   # icp_with_scaling_xyz's statement
    icp = registration_icp_ragged(scaled, (tp, toff), 0.075, inits)
    out = []
    for j in range(s):
        S = np.eye(4)
        S[0, 0], S[1, 1], S[2, 2] = cands[j][best[j]]
        out.append((S, float(sc[koff[j] + best[j]]), icp[j][0]))
    return out


# ---------------------------------------------------------------------------
# reg() over S scans: every stage of stage 2 but the pose initialisation's alignment loop is one pass for all of them.
# ---------------------------------------------------------------------------
def _scan_list(x, s, fn, name):
    """None, or a list of s entries (each a tensor or None) -> a list of s entries."""
    if x is None:
        return [None] * s
    if not isinstance(x, (list, tuple)) or len(x) != s:
        raise ValueError("%s: %s is None or a list of one entry per scan (%d scans)" % (fn, name, s))
    return list(x)


def _voxel_grids(clouds, voxel_size, cols=None):
    """voxel_down_sample_clouds over clouds of which only some bring colours (cols[j] None): the coloured ones in one call, the
    others in another -> (down: list, down_cols: list with None where none was given)."""
    s = len(clouds)
    cols = [None] * s if cols is None else cols
    with_c = [j for j in range(s) if cols[j] is not None]
    without = [j for j in range(s) if cols[j] is None]
    down, dcol = [None] * s, [None] * s
    if with_c:
        d, c = voxel_down_sample_clouds([clouds[j] for j in with_c], voxel_size, colors=[cols[j] for j in with_c])
        for i, j in enumerate(with_c):
            down[j], dcol[j] = d[i], c[i]
    if without:
        for i, d in zip(without, voxel_down_sample_clouds([clouds[j] for j in without], voxel_size)):
            down[i] = d
    return down, dcol


def reg_tensors_scans(partials, completes, generative_model="trellis", dataset="redwood", cd_inv_weight=0.5, diff_init=True,
                      reg_fine_xyz=False, pose_voxel=0.02, cd_only_pose=False, partial_cols=None, complete_cols=None,
                      diff_transforms=None, ragged_pose=False, nn_search=None):
    """``reg_tensors`` for S scans at once: partials / completes are lists of [N_j,3] / [M_j,3] GPU tensors, partial_cols /
    complete_cols / diff_transforms None or lists with one entry per scan (an entry may be None); the other arguments are
    ``reg_tensors``' and hold for every scan.  Returns a list of ``reg_tensors``' dicts, same keys.  The stages:
      pose         the grids at `pose_voxel` of all clouds that need one through ``voxel_down_sample_clouds`` (with colours where
                   given); ``object_pose_optimization`` then runs PER SCAN, unchanged (the default), or -- ``ragged_pose=True`` --
                   the scans that need a pose go through ONE ``object_pose_optimization_scans`` call on the same grids (the
                   ragged alignment loop: the same objective per scan, its gradient summed in another order, so the 200
                   steps agree with the per-scan path in their first steps and in what they converge to, not bit for bit);
                   ``nn_search`` (None, "grid" or "dense") is handed to that call and means nothing without ``ragged_pose``.
                   Entries of diff_transforms that are given are used as they are.
      glue         ``_apply``, ``normalize_numpy`` and the instantmesh rotation are ``reg_tensors``' own statements per scan, so
                   every ragged stage receives the bits ``reg_tensors`` feeds its single-scan stage.
      instantmesh  ``remove_noise_from_point_clouds`` over all sources (its documented caveat: a point whose k-NN mean lies within
                   rounding of the threshold may fall on the other side than ``remove_noise_from_point_cloud`` puts it).
      coarse       the 0.03 grids of all 2 S clouds in one ``voxel_down_sample_clouds`` call, then ``coarse_scale_sweeps``.
      fine         (reg_fine_xyz) the grids in one call -- 0.03 and 0.03, none and 0.04 for pcn / kitti -- then
                   ``iterative_scale_searches`` with [(0.8, 1.2)] * 3, 10.
    Scan j's entry is what ``reg_tensors`` returns on that scan alone, up to the caveats of the ragged stages it goes through
    (coarse_loss: ``coarse_scale_sweeps``' score, a relative few ulp; the ICP bit for bit where the down-sampled target gets
    the one-workgroup plan)."""
    from .optim_registration.diff_obj_pose import object_pose_optimization, object_pose_optimization_scans
    fn = "reg_tensors_scans"
    _lib.check_nn_ragged_search(nn_search, "nn_search")
    if not isinstance(partials, (list, tuple)) or not isinstance(completes, (list, tuple)):
        raise TypeError("%s: partials and completes are lists of [N,3] tensors" % fn)
    s = len(partials)
    if len(completes) != s:
        raise ValueError("%s: %d partials against %d completes" % (fn, s, len(completes)))
    scols = _scan_list(partial_cols, s, fn, "partial_cols")
    tcols = _scan_list(complete_cols, s, fn, "complete_cols")
    diffs = _scan_list(diff_transforms, s, fn, "diff_transforms")
    for name, clouds in (("partials", partials), ("completes", completes)):
        for j, t in enumerate(clouds):
            if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 3:
                raise ValueError("%s: %s[%d] must be an [N,3] tensor" % (fn, name, j))
    _lib.require_gpu(*partials, *completes)
    if s == 0:
        return []
    sources = [t.contiguous().float() for t in partials]
    targets = [t.contiguous().float() for t in completes]
    scols = [None if c is None else c.contiguous().float() for c in scols]
    tcols = [None if c is None else c.contiguous().float() for c in tcols]
    outs = [{} for _ in range(s)]
    if not diff_init:
        diffs = [np.eye(4) for _ in range(s)]
    else:                                                               # :109-122
        need = [j for j in range(s) if diffs[j] is None]
        if need:
            down, dcol = _voxel_grids([targets[j] for j in need] + [sources[j] for j in need], pose_voxel,
                                      [tcols[j] for j in need] + [scols[j] for j in need])
            if ragged_pose:
                n = len(need)
                Ts = object_pose_optimization_scans(down[:n], down[n:], radius=0.02, lr=0.01, iters=200, render_size=224, cd_only=cd_only_pose,
                                                    complete_cols=dcol[:n], partial_cols=dcol[n:], nn_search=nn_search)
                for i, j in enumerate(need):
                    diffs[j] = np.linalg.inv(Ts[i].astype(np.float64))
            for i, j in enumerate([] if ragged_pose else need):
                k = len(need) + i
                # (the loop gets tensors of its own, as voxel_down_sample would hand it: the grids are views of one packed result)
                T = object_pose_optimization(down[i].clone(), down[k].clone(), radius=0.02, lr=0.01, iters=200, render_size=224, cd_only=cd_only_pose,
                                             complete_col=None if dcol[i] is None else dcol[i].clone(),
                                             partial_col=None if dcol[k] is None else dcol[k].clone())
                diffs[j] = np.linalg.inv(T.astype(np.float64))
    for j in range(s):
        outs[j]["diff_transform"] = diffs[j]
        sources[j] = _apply(diffs[j], sources[j])                       # :126
        targets[j], _, _ = normalize_numpy(targets[j], range=0.5)       # :130
    if generative_model in ("instantmesh",):                            # :132-137
        sources, keeps = remove_noise_from_point_clouds(sources)
        for j in range(s):
            if scols[j] is not None:
                scols[j] = scols[j][keeps[j]]
            dev = targets[j].device
            targets[j] = (targets[j].double() @ torch.as_tensor(get_rotate_matrix("x", 90).T, device=dev)
                          @ torch.as_tensor(get_rotate_matrix("y", 90).T, device=dev)).float()
    down = voxel_down_sample_clouds(list(sources) + list(targets), 0.03)
    sweeps = coarse_scale_sweeps(down[:s], down[s:], cd_inv_weight=cd_inv_weight)              # :146-173
    coarse = []
    for j in range(s):
        best_scale, best_loss, T = sweeps[j]
        coarse.append(T)
        outs[j].update(best_scale=best_scale, coarse_loss=best_loss, coarse_transformation=T)
    if reg_fine_xyz:                                                    # :176-199
        sources = [_apply(coarse[j], sources[j]) for j in range(s)]
        if dataset in ("pcn", "kitti"):
            src_s, tgt_s = sources, voxel_down_sample_clouds(list(targets), 0.04)
        else:
            down = voxel_down_sample_clouds(list(sources) + list(targets), 0.03)
            src_s, tgt_s = down[:s], down[s:]
        fine = iterative_scale_searches(list(src_s), list(tgt_s), [(0.8, 1.2)] * 3, 10, cd_inv_weight=cd_inv_weight)
        for j in range(s):
            S, loss_xyz, T_xyz = fine[j]
            outs[j].update(best_scales_transformation=S, xyz_loss=loss_xyz, best_transformation_xyz=T_xyz)
            targets[j] = _apply(np.linalg.inv(S), targets[j])
            targets[j] = _apply(np.linalg.inv(T_xyz), targets[j])
            sources[j] = _apply(np.linalg.inv(coarse[j]), sources[j])
    for j in range(s):
        target = _apply(np.linalg.inv(coarse[j]), targets[j])           # :201-205
        target = _apply(np.linalg.inv(diffs[j]), target)
        source = _apply(np.linalg.inv(diffs[j]), sources[j])
        outs[j].update(source=source, target=target, source_col=scols[j], target_col=tcols[j])
    return outs


def reg_scans(cfg, flags, cd_inv_weight=0.5, diff_init=True, reg_fine_xyz=False, seed=None, ragged_pose=False, nn_search=None, **kwargs):
    """The file form of ``reg`` for a list of flags: returns a list of ``reg``'s dicts and writes every ``{flag}_fused.ply`` WITH
    COLOURS.  Every flag's two input files are checked first: a missing one raises FileNotFoundError naming it before any work.
    With an int ``seed`` ONE draw of 163 840 samples per mesh serves both of ``reg``'s samplings, all meshes in one
    ``sample_surfaces_gpu`` call: sample i does not depend on the count, so the first 120 000 samples, voxel-down-sampled at 0.02
    with their colours (one ``voxel_down_sample_clouds`` call for all meshes), ARE the cloud ``object_pose_optimization``'s file
    form builds.  The partial cloud of the pose comes through ``load_point_cloud`` and the pose runs in tensor form on those
    tensors, per flag (the default), or -- ``ragged_pose=True`` -- for all flags in ONE ``object_pose_optimization_scans`` call on the
    same clouds (the ragged alignment loop; the switch is handed on to ``reg_tensors_scans``, and so is ``nn_search`` -- None, "grid" or
    "dense": that call's nearest-neighbour search).  With ``seed=None`` the host sampler runs per flag, as in
    ``reg`` (``rng=`` included).  Then ``reg_tensors_scans`` and ``fuse_scans`` with ``reg``'s parameters.  The pose's
    debugging files in the working directory (``partial.png``, ``partial_mask.png``, ``final_transform.npy``) are NOT written.
    kwargs: ``cd_only_pose`` and ``rng``, as in ``reg``; anything else raises."""
    import os
    from .optim_registration.diff_obj_pose import load_point_cloud, object_pose_optimization, object_pose_optimization_scans
    from .utils.dataUtils import read_ply, save_ply_xyzrgb
    from .utils.mesh_io import glb2point, load_glb, sample_surfaces_gpu
    _check_file_form_options("reg_scans(cfg, flags, ...)", "it", seed, kwargs)
    _lib.check_nn_ragged_search(nn_search, "nn_search")
    if isinstance(flags, str) or not isinstance(flags, (list, tuple)):
        raise TypeError("reg_scans(cfg, flags, ...): flags is a list of flags")
    path = cfg.output_path
    plys = [f"{path}/{flag}/color_point.ply" for flag in flags]
    glbs = [f"{path}/{flag}/{flag}_{cfg.generative_model}.glb" for flag in flags]
    for f in [x for pair in zip(plys, glbs) for x in pair]:
        if not os.path.exists(f):
            print(f"Path {f} does not exist.")
            raise FileNotFoundError(f"Path {f} does not exist.")
    s = len(flags)
    if s == 0:
        return []
    dev = torch.device(getattr(cfg, "device", "cuda"))
    if seed is not None:
        meshes = []
        for g in glbs:
            V, F, C = load_glb(g)
            meshes.append((V, F, np.full(V.shape, 0.5) if C is None else C))     # (a colourless file: 0.5 grey, as glb2point_gpu)
        drawn = sample_surfaces_gpu(meshes, 163840, int(seed), device=dev)
        txyz, tcol = [d[0] for d in drawn], [d[2] for d in drawn]
    else:
        txyz, tcol = [], []
    diffs = [None] * s
    if diff_init:                                                       # :109-122
        if seed is not None:
            cxyz, ccol = voxel_down_sample_clouds([t[:120000] for t in txyz], 0.02, colors=[c[:120000] for c in tcol])
        pose_clouds = []
        for j in range(s):
            pxyz, pcol = load_point_cloud(plys[j], dev, radius=0.02, num_points=8000)
            if seed is not None:
                cx, cc = cxyz[j].clone(), ccol[j].clone()
            else:
                cx, cc = load_point_cloud(glbs[j], dev, radius=0.02, num_points=120000)
            if ragged_pose:
                pose_clouds.append((cx, cc, pxyz, pcol))
                continue
            T = object_pose_optimization(cx, pxyz, radius=0.02, lr=0.01, iters=200, render_size=224, vis=True,
                                         cd_only=kwargs.get("cd_only_pose", False), complete_col=cc, partial_col=pcol)
            diffs[j] = np.linalg.inv(T.astype(np.float64))
        if ragged_pose:
            Ts = object_pose_optimization_scans([q[0] for q in pose_clouds], [q[2] for q in pose_clouds], radius=0.02, lr=0.01, iters=200,
                                                render_size=224, cd_only=kwargs.get("cd_only_pose", False),
                                                complete_cols=[q[1] for q in pose_clouds], partial_cols=[q[3] for q in pose_clouds],
                                                nn_search=nn_search)
            diffs = [np.linalg.inv(T.astype(np.float64)) for T in Ts]
    sxyz, scol = [], []
    for j in range(s):
        xyz, col = read_ply(plys[j])                                    # :124 o3d.io.read_point_cloud
        if seed is None:
            t, c = glb2point(glbs[j], num_points=163840, rng=kwargs.get("rng"))                # :125
            txyz.append(torch.as_tensor(t, dtype=torch.float32, device=dev))
            tcol.append(torch.as_tensor(c, dtype=torch.float32, device=dev))
        if col is None:
            col = np.zeros_like(xyz)                                    # an open3d cloud without colours: fused file stays valid
        sxyz.append(torch.as_tensor(xyz, dtype=torch.float32, device=dev))
        scol.append(torch.as_tensor(col, dtype=torch.float32, device=dev))
    outs = reg_tensors_scans(sxyz, txyz, generative_model=cfg.generative_model, dataset=getattr(cfg, "dataset", "redwood"),
                             cd_inv_weight=cd_inv_weight, diff_init=diff_init, reg_fine_xyz=reg_fine_xyz, partial_cols=scol,
                             complete_cols=tcol, diff_transforms=diffs if diff_init else None, ragged_pose=ragged_pose, nn_search=nn_search)
    fused = fuse_scans([o["source"] for o in outs], [o["target"] for o in outs], num_points=20000, distance_threshold=0.0001,
                       std_ratio=2.5, source_cols=[o["source_col"] for o in outs], target_cols=[o["target_col"] for o in outs])   # :207-217
    for j, flag in enumerate(flags):
        outs[j].update(fused=fused[j][0], fused_col=fused[j][1], fused_path=f"{path}/{flag}/{flag}_fused.ply")
        save_ply_xyzrgb(fused[j][0].double().cpu().numpy(), fused[j][1].double().cpu().numpy(), outs[j]["fused_path"])     # :221
    return outs
