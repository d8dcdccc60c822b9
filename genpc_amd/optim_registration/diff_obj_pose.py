"""The SE(3)+scale alignment loop of the reference's
optim_registration/diff_obj_pose.py on the gfx950 library.

``object_pose_optimization`` keeps the reference's name, signature, hyper-parameters and
return value (4x4 numpy ``[[sR, t],[0,1]]``, :464-468,:496-594): called with the GLB and PLY
paths it loads both clouds WITH THEIR COLOURS like the reference's load_point_cloud (:136-164);
called with tensors it skips the file layer.  It optimises the reference's objective
``mask_loss + 3 * (partial_l1(pts, partial) + 0.5 partial_l1(partial, pts)) + 1e-3 |RR^T - I|_F``
(:329-333,543-546).  ``mask_loss`` (30 MSE + BCE + 10 Dice on sigmoid soft masks of the
statistically normalised images, :204-217,261-311) is the reference's own torch code
restated (and pinned to it: tests/golden/ref_py_mask_loss.npz).  The IMAGES: the reference draws
them with pytorch3d's CUDA-only Pulsar renderer (absent here, unpinned); this build restates
Pulsar's PUBLISHED blending function -- a softmax in depth over the discs covering a pixel, with
the reference's gamma 1e-2, znear 1e-4, zfar 5, background 0 -- on its own disc footprint and
camera (``render_tune(1)``, the default since round 5; what of it is from memory is listed in
oracle/genpc_oracle_geom.c and include/genpc_hip.h).  ``render_tune(0)`` selects the coverage
splat of rounds 2-4 (occupancy times the coverage-weighted mean colour: order-independent,
front and back surfaces averaged).  The whole multi-start loop
runs on the device without host synchronisation (7 launches per Adam step; 4 with
``cd_only=True``).
"""
import torch

from .. import _lib

_L = _lib.lib
_p = _lib.ptr


def pose_transform(vert_pos, center, params):
    """ObjectPoseOptim.forward's point map (:419-423).  params = rot_6d|trans|log_scale."""
    vert_pos = vert_pos.contiguous().float()
    center = center.contiguous().float()
    params = params.contiguous().float()
    _lib.check_tensors((("vert_pos", vert_pos), ("center", center), ("params", params)))
    pts = torch.empty_like(vert_pos)
    rc = _lib.on_device_of(vert_pos, _L.genpc_pose_transform, vert_pos.shape[0], _p(vert_pos), _p(center),
                           _p(params), _p(pts))
    if rc != 1:
        raise RuntimeError("genpc_pose_transform failed: " + _lib.last_error())
    return pts


def nn_seeded_step(rest, center, params, static, seed1, seed2, sample=1, d1=None, d2=None):
    """One step of the loop's seeded nearest-neighbour search (genpc_nn_seeded_step) for B elements: rest [B,nm,3],
    center [B,3], params [B,10], static [B,ns,3]; seed1 [B,nm] / seed2 [B,ns] int32 are last step's answers (a value
    outside the target count is no seed) and are NOT modified.  -> (posed [B,nm,3], d1, i1 [B,nm], d2, i2 [B,ns]).
    sample > 1: only every sample-th block of queries is answered; the others keep d1 / d2 as given (empty if None) and
    their seeds."""
    _lib.check_tensors((("rest", rest), ("center", center), ("params", params), ("static", static)), (("seed1", seed1), ("seed2", seed2)))
    if rest.dim() != 3 or rest.shape[2] != 3 or static.dim() != 3 or static.shape[2] != 3:
        raise ValueError("nn_seeded_step: clouds must be [B,N,3], got %s and %s" % (tuple(rest.shape), tuple(static.shape)))
    b, nm, ns = rest.shape[0], rest.shape[1], static.shape[1]
    if static.shape[0] != b or tuple(center.shape) != (b, 3) or tuple(params.shape) != (b, 10) or tuple(seed1.shape) != (b, nm) \
            or tuple(seed2.shape) != (b, ns):
        raise ValueError("nn_seeded_step: shapes differ: rest %s, center %s, params %s, static %s, seeds %s and %s"
                         % (tuple(rest.shape), tuple(center.shape), tuple(params.shape), tuple(static.shape), tuple(seed1.shape), tuple(seed2.shape)))
    posed = torch.empty_like(rest)
    i1, i2 = seed1.clone(), seed2.clone()
    d1 = torch.empty(b, nm, device=rest.device) if d1 is None else d1.clone()
    d2 = torch.empty(b, ns, device=rest.device) if d2 is None else d2.clone()
    _lib.check_tensors((("d1", d1), ("d2", d2)))
    rc = _lib.on_device_of(rest, _L.genpc_nn_seeded_step, b, nm, _p(rest), _p(center), _p(params), ns, _p(static), _p(posed),
                           _p(d1), _p(i1), _p(d2), _p(i2), int(sample))
    if rc != 1:
        raise RuntimeError("genpc_nn_seeded_step failed (rc=%d): %s" % (rc, _lib.last_error()))
    return posed, d1, i1, d2, i2


def pose_cd_loss_grad(vert_pos, center, params, partial, cd_weight=3.0, reg_weight=0.001):
    """-> (loss[3] = total, cd, |RR^T-I|_F ; grad[10]) for the current parameters."""
    from .. import chamfer_3D
    vert_pos = vert_pos.contiguous().float()
    partial = partial.contiguous().float()
    pts = pose_transform(vert_pos, center, params)
    nc, np_ = vert_pos.shape[0], partial.shape[0]
    dev = vert_pos.device
    d1 = torch.empty(1, nc, device=dev)
    d2 = torch.empty(1, np_, device=dev)
    i1 = torch.empty(1, nc, device=dev, dtype=torch.int32)
    i2 = torch.empty(1, np_, device=dev, dtype=torch.int32)
    if chamfer_3D.forward(pts[None], partial[None], d1, d2, i1, i2) != 1:
        raise RuntimeError("chamfer forward failed: " + _lib.last_error())
    loss = torch.empty(3, device=dev)
    grad = torch.empty(10, device=dev)
    rc = _lib.on_device_of(vert_pos, _L.genpc_pose_cd_grad, nc, _p(vert_pos), _p(center.contiguous().float()),
                           _p(params.contiguous().float()), np_, _p(partial), _p(d1), _p(i1), _p(d2), _p(i2),
                           float(cd_weight), float(reg_weight), _p(loss), _p(grad))
    if rc != 1:
        raise RuntimeError("genpc_pose_cd_grad failed: " + _lib.last_error())
    return loss, grad


def _col(colors, like, name):
    """optional [..,N,3] colours in [0,1] -> contiguous float32 on like's device (None stays None = white)."""
    if colors is None:
        return None
    c = torch.as_tensor(colors, device=like.device).contiguous().float()
    if c.shape != like.shape:
        raise ValueError("%s must have the shape of its cloud %s, got %s" % (name, tuple(like.shape), tuple(c.shape)))
    return c


def render_tune(blend):
    """The renderer of the mask term for the calling thread: 1 Pulsar's blending function (default), 0 the coverage
    splat, < 0 the default again.  Returns the previous setting (-1 = default)."""
    return int(_L.genpc_render_tune(int(blend)))


def splat_image(points, radius, render_size=224, colors=None):
    """The library's render of a cloud [N,3] (colours [N,3] in [0,1], None = white)
    -> [render_size, render_size, 3] in [0,1] (render_reference_image, diff_obj_pose.py:108-134):
    Pulsar's blending function by default, the coverage splat under render_tune(0); include/genpc_hip.h."""
    pts = points.contiguous().float()
    _lib.check_tensors((("points", pts),))
    col = _col(colors, pts, "colors")
    img = torch.empty(render_size, render_size, 3, device=pts.device)
    rc = _lib.on_device_of(pts, _L.genpc_splat_image, pts.shape[0], _p(pts), _p(col), float(radius), int(render_size), _p(img))
    if rc != 1:
        raise RuntimeError("genpc_splat_image failed (rc=%d): %s" % (rc, _lib.last_error()))
    return img


def compute_mask_from_rendering(rendered_img, threshold=0.1, method="luminance"):
    """diff_obj_pose.py:166-178: hard mask of a render (the second output of render_reference_image)."""
    if rendered_img.shape[-1] == 4:
        return (rendered_img[..., 3] > 0).float()
    if method == "occupancy":
        return (rendered_img.sum(-1) > threshold).float()
    luminance = 0.299 * rendered_img[:, :, 0] + 0.587 * rendered_img[:, :, 1] + 0.114 * rendered_img[:, :, 2]
    return (luminance > threshold).float()


def mask_loss(result, ref_img, with_grad=False):
    """compute_loss_function's mask_loss (diff_obj_pose.py:286-311: per-channel statistical
    normalisation of `result` towards `ref_img`, luminance soft masks, 30 MSE + BCE + 10 Dice) for
    [S,S,3] float32 GPU images, on the library's kernels -> loss (0-dim tensor), and d loss / d result."""
    a = result.contiguous().float()
    r = ref_img.contiguous().float()
    _lib.check_tensors((("result", a), ("ref_img", r)))
    if a.shape != r.shape or a.dim() != 3 or a.shape[2] != 3 or a.shape[0] != a.shape[1]:
        raise ValueError("mask_loss: images must be [S,S,3] and alike, got %s and %s" % (tuple(a.shape), tuple(r.shape)))
    loss = torch.empty(1, device=a.device)
    grad = torch.empty_like(a) if with_grad else None
    rc = _lib.on_device_of(a, _L.genpc_mask_loss, a.shape[0], _p(a), _p(r), _p(loss), _p(grad))
    if rc != 1:
        raise RuntimeError("genpc_mask_loss failed (rc=%d): %s" % (rc, _lib.last_error()))
    return (loss[0], grad) if with_grad else loss[0]


def pose_loss_grad(vert_pos, center, params, partial, radius, render_size=224, cd_weight=3.0, reg_weight=0.001,
                   mask_weight=1.0, vert_col=None, partial_col=None):
    """compute_loss_function + rot_reg for the current parameters
    -> (loss[4] = total, cd, |RR^T-I|_F, mask_loss ; grad[10]).  vert_col / partial_col: the clouds'
    colours ([N,3] in [0,1]; None = white)."""
    from .. import chamfer_3D
    vert_pos = vert_pos.contiguous().float()
    partial = partial.contiguous().float()
    vc, pc = _col(vert_col, vert_pos, "vert_col"), _col(partial_col, partial, "partial_col")
    pts = pose_transform(vert_pos, center, params)
    nc, np_ = vert_pos.shape[0], partial.shape[0]
    dev = vert_pos.device
    d1 = torch.empty(1, nc, device=dev)
    d2 = torch.empty(1, np_, device=dev)
    i1 = torch.empty(1, nc, device=dev, dtype=torch.int32)
    i2 = torch.empty(1, np_, device=dev, dtype=torch.int32)
    if chamfer_3D.forward(pts[None], partial[None], d1, d2, i1, i2) != 1:
        raise RuntimeError("chamfer forward failed: " + _lib.last_error())
    loss = torch.empty(4, device=dev)
    grad = torch.empty(10, device=dev)
    rc = _lib.on_device_of(vert_pos, _L.genpc_pose_loss_grad, nc, _p(vert_pos), _p(vc), _p(center.contiguous().float()),
                           _p(params.contiguous().float()), np_, _p(partial), _p(pc), _p(d1), _p(i1), _p(d2), _p(i2),
                           float(cd_weight), float(reg_weight), float(mask_weight), float(radius), int(render_size),
                           _p(loss), _p(grad))
    if rc != 1:
        raise RuntimeError("genpc_pose_loss_grad failed (rc=%d): %s" % (rc, _lib.last_error()))
    return loss, grad


def pose_loss_grad_batch(vert_pos, center, params, partial, radius, render_size=224, cd_weight=3.0, reg_weight=0.001,
                         mask_weight=1.0, vert_col=None, partial_col=None):
    """pose_loss_grad for B elements in one call, each with its own clouds, centre and parameters: vert_pos [B,nc,3],
    center [B,3], params [B,10], partial [B,np,3] -> (loss[B,4], grad[B,10]).  The launches are those of one step of
    object_pose_optimization's loop at B elements (nearest neighbours included), so the kernel forms the loop selects
    for wide calls are evaluated; no Adam step is taken.  mask_weight = 0: the Chamfer-only objective."""
    vert_pos = vert_pos.contiguous().float()
    partial = partial.contiguous().float()
    center = center.contiguous().float()
    params = params.contiguous().float()
    _lib.check_tensors((("vert_pos", vert_pos), ("center", center), ("params", params), ("partial", partial)))
    if vert_pos.dim() != 3 or vert_pos.shape[2] != 3 or partial.dim() != 3 or partial.shape[2] != 3:
        raise ValueError("pose_loss_grad_batch: clouds must be [B,N,3], got %s and %s" % (tuple(vert_pos.shape), tuple(partial.shape)))
    b, nc, np_ = vert_pos.shape[0], vert_pos.shape[1], partial.shape[1]
    if partial.shape[0] != b or tuple(center.shape) != (b, 3) or tuple(params.shape) != (b, 10):
        raise ValueError("pose_loss_grad_batch: batch sizes differ: vert_pos %s, center %s, params %s, partial %s"
                         % (tuple(vert_pos.shape), tuple(center.shape), tuple(params.shape), tuple(partial.shape)))
    vc, pc = _col(vert_col, vert_pos, "vert_col"), _col(partial_col, partial, "partial_col")
    loss = torch.empty(b, 4, device=vert_pos.device)
    grad = torch.empty(b, 10, device=vert_pos.device)
    rc = _lib.on_device_of(vert_pos, _L.genpc_pose_loss_grad_batch, b, nc, _p(vert_pos), _p(vc), _p(center), _p(params), np_,
                           _p(partial), _p(pc), float(cd_weight), float(reg_weight), float(mask_weight), float(radius),
                           int(render_size), _p(loss), _p(grad))
    if rc != 1:
        raise RuntimeError("genpc_pose_loss_grad_batch failed (rc=%d): %s" % (rc, _lib.last_error()))
    return loss, grad


RAGGED_MAX_ELEMENTS = 384          # genpc_hip.h GENPC_POSE_RAGGED_MAX_ELEMENTS: scans x starts of one library call


def pose_scan_chunks(scans, starts, limit=RAGGED_MAX_ELEMENTS):
    """The library calls a list of `scans` scans at `starts` starts each is cut into: [(first, end)] scan ranges of at most
    limit // starts scans (97 scans at 4 starts: (0, 96) and (96, 97))."""
    if starts < 1:
        raise ValueError("pose_scan_chunks: starts must be at least 1, got %d" % starts)
    per = limit // starts
    if per < 1:
        raise ValueError("pose_scan_chunks: %d starts do not fit the %d elements of a call" % (starts, limit))
    return [(a, min(a + per, scans)) for a in range(0, scans, per)]


def _ragged_clouds(clouds, fn, name, what):
    """A list of [N_j,3] GPU tensors or packed (points, offsets) -> (points [T,3], offsets); a CPU tensor and an empty cloud raise,
    naming the scan."""
    from .. import _ragged
    if not _ragged.is_packed(clouds) and isinstance(clouds, (list, tuple)):
        for j, t in enumerate(clouds):
            if torch.is_tensor(t) and not t.is_cuda:
                raise RuntimeError("%s: GPU tensors only (%s[%d], scan %d, is a %s tensor); the HIP path has no CPU fallback" % (fn, name, j, j, t.device))
    points, off = _ragged.ragged_side(clouds, fn, name)
    if len(off) > 1 and not points.is_cuda:
        raise RuntimeError("%s: GPU tensors only (%s is a %s tensor); the HIP path has no CPU fallback" % (fn, name, points.device))
    for j in range(len(off) - 1):
        if off[j + 1] == off[j]:
            raise ValueError("%s: scan %d has an empty %s cloud" % (fn, j, what))
    return points, off


def _ragged_colours(cols, points, off, fn, name):
    """None, or a list with one entry per scan ([N_j,3] in [0,1], or None = white) -> packed [T,3] float32 or None."""
    if cols is None:
        return None
    s = len(off) - 1
    if not isinstance(cols, (list, tuple)) or len(cols) != s:
        raise ValueError("%s: %s must be None or a list with one entry per scan (%d), got %s"
                         % (fn, name, s, len(cols) if isinstance(cols, (list, tuple)) else type(cols).__name__))
    if all(c is None for c in cols):
        return None
    out = torch.ones_like(points)
    for j, c in enumerate(cols):
        if c is None:
            continue
        n = off[j + 1] - off[j]
        c = torch.as_tensor(c)
        if tuple(c.shape) != (n, 3):
            raise ValueError("%s: %s[%d] must have the shape of scan %d's cloud (%d, 3), got %s" % (fn, name, j, j, n, tuple(c.shape)))
        out[off[j]:off[j + 1]] = c.to(device=points.device, dtype=torch.float32)
    return out


def pose_loss_grad_ragged(vert_pos, center, params, partial, radius, render_size=224, cd_weight=3.0, reg_weight=0.001,
                          mask_weight=1.0, vert_col=None, partial_col=None, nn_search=None):
    """pose_loss_grad_batch for c elements of DIFFERENT sizes in one call (genpc_pose_loss_grad_ragged): vert_pos / partial are
    lists of [N_j,3] GPU tensors or packed (points, offsets), center [c,3], params [c,10], vert_col / partial_col None or lists
    with one entry per element -> (loss[c,4], grad[c,10]).  The launches are one step of object_pose_optimization_scans' loop;
    no Adam step is taken.  mask_weight = 0: the Chamfer-only objective.  More than 384 elements go in several calls.
    nn_search: None (the calling thread's ragged search, the grid search by default), "grid" or "dense" (all pairs: the same
    bits) for the step's two nearest-neighbour searches."""
    from .. import _ragged
    fn = "pose_loss_grad_ragged"
    _lib.check_nn_ragged_search(nn_search, "nn_search")
    cpts, coff = _ragged_clouds(vert_pos, fn, "vert_pos", "complete")
    ppts, poff = _ragged_clouds(partial, fn, "partial", "partial")
    c = len(coff) - 1
    if len(poff) - 1 != c:
        raise ValueError("%s: %d complete clouds against %d partial clouds" % (fn, c, len(poff) - 1))
    center = center.contiguous().float()
    params = params.contiguous().float()
    _lib.check_tensors((("center", center), ("params", params)))
    if tuple(center.shape) != (c, 3) or tuple(params.shape) != (c, 10):
        raise ValueError("%s: center must be [%d,3] and params [%d,10], got %s and %s" % (fn, c, c, tuple(center.shape), tuple(params.shape)))
    vc, pc = _ragged_colours(vert_col, cpts, coff, fn, "vert_col"), _ragged_colours(partial_col, ppts, poff, fn, "partial_col")
    loss = torch.empty(c, 4, device=center.device)
    grad = torch.empty(c, 10, device=center.device)
    for a, b, co, po in _ragged.chunks(RAGGED_MAX_ELEMENTS, coff, poff):
        _, cp = _ragged.host_ints(co, "coff")
        _, pp = _ragged.host_ints(po, "poff")
        with _lib.nn_ragged_search(nn_search, "nn_search"):
            rc = _lib.on_device_of(cpts, _L.genpc_pose_loss_grad_ragged, b - a, cp, pp, _p(cpts[coff[a]:coff[b]]),
                                   _p(None if vc is None else vc[coff[a]:coff[b]]), _p(center[a:b]), _p(params[a:b]), _p(ppts[poff[a]:poff[b]]),
                                   _p(None if pc is None else pc[poff[a]:poff[b]]), float(cd_weight), float(reg_weight), float(mask_weight),
                                   float(radius), int(render_size), _p(loss[a:b]), _p(grad[a:b]))
        if rc != 1:
            raise RuntimeError("genpc_pose_loss_grad_ragged failed (rc=%d): %s" % (rc, _lib.last_error()))
    return loss, grad


def object_pose_optimization_scans(completes, partials, radius=0.005, lr=0.005, iters=300, render_size=224, cam_bias_num=4,
                                   return_history=False, cd_only=False, complete_cols=None, partial_cols=None, nn_search=None):
    """object_pose_optimization's tensor form for S scans of DIFFERENT sizes in one call (genpc_pose_optimize_ragged): completes /
    partials are lists of [N_j,3] GPU tensors or packed (points, offsets), complete_cols / partial_cols None or lists with one
    entry per scan (an entry may be None = white).  Returns a list of S 4x4 numpy ``[[sR, t],[0,1]]``; with return_history
    also a list of [cam_bias_num, iters + 1] loss histories and a list of [10] parameters.  Scan j's results are those of
    object_pose_optimization on scan j alone up to the summation order of its gradient (tests/test_gpu_pose_ragged_loop.py).
    The starts run side by side as batch elements; a library call holds 384 of them (96 scans at 4 starts), a longer list goes
    in several calls (pose_scan_chunks); ONE read-back at the end.  A CPU tensor, lists of different lengths, a colour list of
    the wrong length or shape and an empty cloud raise, naming the scan.
    nn_search: None (the calling thread's ragged search, the grid search by default), "grid" or "dense" -- every step's two
    nearest-neighbour searches by all pairs (csrc/nn_ragged_dense.hip): the same bits, at a cost that does not depend on how
    well a start is aligned, and no grid is built."""
    from .. import _ragged
    fn = "object_pose_optimization_scans"
    _lib.check_nn_ragged_search(nn_search, "nn_search")
    cpts, coff = _ragged_clouds(completes, fn, "completes", "complete")
    ppts, poff = _ragged_clouds(partials, fn, "partials", "partial")
    s = len(coff) - 1
    if len(poff) - 1 != s:
        raise ValueError("%s: %d complete clouds against %d partial clouds" % (fn, s, len(poff) - 1))
    cc, pc = _ragged_colours(complete_cols, cpts, coff, fn, "complete_cols"), _ragged_colours(partial_cols, ppts, poff, fn, "partial_cols")
    starts, iters = int(cam_bias_num), int(iters)
    ranges = pose_scan_chunks(s, starts)
    if s == 0:
        return ([], [], []) if return_history else []
    if cpts.device != ppts.device:
        raise ValueError("%s: completes are on %s, partials on %s" % (fn, cpts.device, ppts.device))
    _lib.check_tensors((("completes", cpts), ("partials", ppts)))
    hlen = starts * (iters + 1)
    out = torch.empty(s, 16 + hlen + 10, device=cpts.device)          # one block: one read-back
    T, hist, bp = out[:, :16], out[:, 16:16 + hlen], out[:, 16 + hlen:]
    for a, b in ranges:
        tt = torch.empty(b - a, 16, device=cpts.device)
        hh = torch.empty(b - a, hlen, device=cpts.device)
        pp = torch.empty(b - a, 10, device=cpts.device)
        _, cp = _ragged.host_ints([v - coff[a] for v in coff[a:b + 1]], "coff")
        _, pq = _ragged.host_ints([v - poff[a] for v in poff[a:b + 1]], "poff")
        with _lib.nn_ragged_search(nn_search, "nn_search"):
            rc = _lib.on_device_of(cpts, _L.genpc_pose_optimize_ragged, b - a, cp, pq, _p(cpts[coff[a]:coff[b]]),
                                   _p(None if cc is None else cc[coff[a]:coff[b]]), _p(ppts[poff[a]:poff[b]]),
                                   _p(None if pc is None else pc[poff[a]:poff[b]]), float(lr), iters, starts, float(radius), int(render_size),
                                   0.0 if cd_only else 1.0, _p(tt), _p(hh), _p(pp))
        if rc != 1:
            raise RuntimeError("genpc_pose_optimize_ragged failed (rc=%d): %s" % (rc, _lib.last_error()))
        T[a:b], hist[a:b], bp[a:b] = tt, hh, pp
    host = out.cpu().numpy()
    transforms = [host[j, :16].reshape(4, 4).copy() for j in range(s)]
    if not return_history:
        return transforms
    return (transforms, [host[j, 16:16 + hlen].reshape(starts, iters + 1).copy() for j in range(s)],
            [host[j, 16 + hlen:].copy() for j in range(s)])


def load_point_cloud(point_path, device, radius=0.05, num_points=5000):
    """diff_obj_pose.py:136-164: a .ply through load_xyz, a .glb through glb2point, both voxel
    down-sampled at `radius` WITH their colours -> (vert_pos [N,3], vert_col [N,3] in [0,1]) on
    `device`.  (load_xyz substitutes position-derived colours for a colourless PLY, glb2point grey
    for a colourless mesh, so vert_col is never None -- as in the reference.)"""
    from ..utils.dataUtils import load_xyz
    from ..utils.mesh_io import glb2point
    if point_path.endswith(".ply"):
        xyz, color = load_xyz(point_path, down_sample=radius, device=device)
    elif point_path.endswith(".glb"):
        xyz, color = glb2point(point_path, down_sample=radius, num_points=num_points, device=device)
    else:
        raise ValueError("Unsupported point cloud format")
    vert_pos = torch.as_tensor(xyz, dtype=torch.float32, device=device)
    if color is None:
        vert_col = torch.ones(vert_pos.shape[0], 3, dtype=torch.float32, device=device)
    else:
        vert_col = torch.as_tensor(color, dtype=torch.float32, device=device)
        if vert_col.max() > 1.0:
            vert_col = vert_col / 255.0
    return vert_pos, vert_col


def object_pose_optimization(glb_path, point_path, radius=0.005, lr=0.005, iters=300, render_size=224,
                             vis=False, save_path=None, device=None, cam_bias_num=4, return_history=False,
                             cd_only=False, complete_col=None, partial_col=None, seed=None):
    """diff_obj_pose.py:496-594, same positional arguments and hyper-parameters, returns the 4x4 numpy
    ``[[sR, t],[0,1]]`` (:464-468).

    File form (the reference's): ``glb_path`` / ``point_path`` are paths; the complete cloud is
    sampled from the GLB (120 000 points) and the partial cloud read from the PLY (both voxel
    down-sampled at ``radius`` with their colours, load_point_cloud); ``seed`` (an int, file form only) draws those
    samples on the device, reproducibly (utils/mesh_io.glb2point_gpu).
    Tensor form: ``glb_path`` = complete_xyz [Nc,3] and ``point_path`` = partial_xyz [Np,3] GPU
    tensors -- or [B,Nc,3] / [B,Np,3]: B scans optimised in lock-step, one batched NN launch per Adam
    step (returns [B,4,4]) -- with their colours in ``complete_col`` / ``partial_col`` (None = white).

    radius / render_size parameterise the silhouette term (splat radius in world units, image side);
    cd_only=True drops that term (Chamfer + orthogonality only).  vis / save_path (the reference's
    debug GIF) are accepted and unused.  The file form also leaves the reference's side-effect files in
    the working directory: ``partial.png``, ``partial_mask.png`` (:508-509) and ``final_transform.npy``
    (:591).  A start stops early after 300 steps without a new best loss (:529-556; never at iters <= 300)."""
    file_form = False
    if isinstance(glb_path, str) or isinstance(point_path, str):
        if not (isinstance(glb_path, str) and isinstance(point_path, str)):
            raise TypeError("object_pose_optimization: pass two paths or two tensors")
        if device is None:
            device = torch.device("cuda:0")
        partial_xyz, partial_col = load_point_cloud(point_path, device, radius=radius, num_points=8000)      # :502
        if seed is None:
            complete_xyz, complete_col = load_point_cloud(glb_path, device, radius=radius, num_points=120000)   # :504
        else:                              # the same cloud drawn on the device, reproducibly (colours are in [0,1] already)
            from ..utils.mesh_io import glb2point_gpu
            if not glb_path.endswith(".glb"):
                raise ValueError("Unsupported point cloud format")
            complete_xyz, complete_col = glb2point_gpu(glb_path, down_sample=radius, num_points=120000, seed=seed, device=device)
        file_form = True
    else:
        if seed is not None:
            raise TypeError("object_pose_optimization: seed belongs to the file form (the tensor form samples nothing)")
        complete_xyz, partial_xyz = glb_path, point_path
    batched = complete_xyz.dim() == 3
    complete_xyz = (complete_xyz if batched else complete_xyz[None]).contiguous().float()
    partial_xyz = (partial_xyz if batched else partial_xyz[None]).contiguous().float()
    _lib.check_tensors((("complete_xyz", complete_xyz), ("partial_xyz", partial_xyz)))
    if complete_xyz.shape[0] != partial_xyz.shape[0]:
        raise ValueError("object_pose_optimization: batch sizes differ")
    if complete_col is not None and not batched:
        complete_col = torch.as_tensor(complete_col)[None]
    if partial_col is not None and not batched:
        partial_col = torch.as_tensor(partial_col)[None]
    cc, pc = _col(complete_col, complete_xyz, "complete_col"), _col(partial_col, partial_xyz, "partial_col")
    if file_form:
        # the reference's side-effect files in the working directory (:508-509): the reference image and its mask
        from PIL import Image
        ref_img = splat_image(partial_xyz[0], radius, render_size, None if pc is None else pc[0])
        ref_mask = compute_mask_from_rendering(ref_img)
        Image.fromarray((ref_img.detach().cpu() * 255).to(torch.uint8).numpy()).save("partial.png")
        Image.fromarray((ref_mask.detach().cpu().numpy() * 255).astype("uint8")).save("partial_mask.png")
    dev = complete_xyz.device
    b = complete_xyz.shape[0]
    T = torch.empty(b, 16, device=dev)
    hist = torch.empty(b, cam_bias_num * (iters + 1), device=dev)
    bp = torch.empty(b, 10, device=dev)
    rc = _lib.on_device_of(complete_xyz, _L.genpc_pose_optimize_batch, b, complete_xyz.shape[1], _p(complete_xyz), _p(cc),
                           partial_xyz.shape[1], _p(partial_xyz), _p(pc), float(lr), int(iters), int(cam_bias_num),
                           float(radius), int(render_size), 0.0 if cd_only else 1.0, _p(T), _p(hist), _p(bp))
    if rc != 1:
        raise RuntimeError("genpc_pose_optimize_batch failed (rc=%d): %s" % (rc, _lib.last_error()))
    final_transform = T.reshape(b, 4, 4).cpu().numpy()
    h = hist.reshape(b, cam_bias_num, iters + 1).cpu().numpy()
    if not batched:
        final_transform, h, bpn = final_transform[0], h[0], bp[0].cpu().numpy()
    else:
        bpn = bp.cpu().numpy()
    if file_form:
        import numpy as np
        np.save("final_transform.npy", final_transform)      # :591
    if return_history:
        return final_transform, h, bpn
    return final_transform
