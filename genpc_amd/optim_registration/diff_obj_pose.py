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

That loop is ONE fixed objective with an analytic gradient.  The reference's stage is a torch program, and the second half of
this file is that program on the library's renderer: ``render_points`` (a ``torch.autograd.Function`` over genpc_render_points /
genpc_render_points_backward, csrc/render_grad.hip), the reference's ``ObjectPoseOptim``, ``render_reference_image``,
``compute_loss_function`` (with ``weights=``), ``normalize_images``, ``compute_soft_mask``, ``dice_loss``, ``soft_iou_loss``,
``edge_loss``, ``get_init_rot``, ``build_transform`` restated from their formulas, and ``object_pose_optimization_torch``, its
Adam loop with an objective the caller may replace (``loss_fn=``).  DESIGN.md 4.5d.

``render_points_ragged`` is that operation for S clouds of different sizes in one call, each with a radius of its own
(genpc_render_points_ragged / genpc_render_points_ragged_backward), and with ``cameras=(R, T, focal)`` for other pinhole cameras
than the library's one: ``camera_points`` maps the points into the library's camera frame in plain torch (so R and T get
gradients from autograd) and the radius is scaled by focal / 4.  ``look_at_view_transform``, ``render_reference_images`` and
``ObjectPoseOptimViews`` (one posed cloud under V cameras) stand on it.  DESIGN.md 4.5e.
"""
import ctypes
import math

import torch
from torch import nn

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


# ------------------------------------------------------------------------------------------------------------------------------
# The customisable path: the renderer as a torch.autograd.Function, the reference's torch helpers restated from their formulas,
# its nn.Module and its Adam loop in torch.  object_pose_optimization above stays the fast path (one fused analytic-gradient
# loop of ONE objective); what follows lets a caller change the objective, optimise points or colours, or put the rendered
# image into an autograd graph of their own.

def _thread_blend():
    """the calling thread's render_tune mode as 0 / 1 (read by setting the default and putting back what was there)"""
    prev = int(_L.genpc_render_tune(-1))
    _L.genpc_render_tune(prev)
    return 0 if prev == 0 else 1


def render_points_forward(pts, col, radius, render_size, blend):
    """genpc_render_points on [B,N,3] float32 GPU tensors (col None: white) -> (img [B,S,S,3], planes [B,5,S*S])."""
    b, n, s = pts.shape[0], pts.shape[1], int(render_size)
    img = torch.empty(b, s, s, 3, device=pts.device)
    planes = torch.empty(b, 5, s * s, device=pts.device)
    rc = _lib.on_device_of(pts, _L.genpc_render_points, b, n, _p(pts), _p(col), float(radius), s, int(blend), _p(img), _p(planes))
    if rc != 1:
        raise RuntimeError("genpc_render_points failed (rc=%d): %s" % (rc, _lib.last_error()))
    return img, planes


def render_points_backward(pts, col, radius, render_size, blend, planes, grad_img, want_col=True):
    """genpc_render_points_backward: planes as render_points_forward returned them for the same arguments, grad_img [B,S,S,3]
    -> (grad_pts [B,N,3], grad_col [B,N,3] or None)."""
    b, n = pts.shape[0], pts.shape[1]
    grad_pts = torch.zeros_like(pts) if n == 0 else torch.empty_like(pts)
    grad_col = (torch.zeros_like(pts) if n == 0 else torch.empty_like(pts)) if want_col else None
    rc = _lib.on_device_of(pts, _L.genpc_render_points_backward, b, n, _p(pts), _p(col), float(radius), int(render_size), int(blend),
                           _p(planes), _p(grad_img), _p(grad_pts), _p(grad_col))
    if rc != 1:
        raise RuntimeError("genpc_render_points_backward failed (rc=%d): %s" % (rc, _lib.last_error()))
    return grad_pts, grad_col


class _RenderPoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts, col, radius, render_size, blend):
        img, planes = render_points_forward(pts, col, radius, render_size, blend)
        if col is None:
            ctx.save_for_backward(pts, planes)
        else:
            ctx.save_for_backward(pts, planes, col)
        ctx.args = (float(radius), int(render_size), int(blend))      # (the blend of the FORWARD: the backward's thread has a mode of its own)
        return img

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_img):
        saved = ctx.saved_tensors
        pts, planes, col = saved[0], saved[1], saved[2] if len(saved) > 2 else None
        radius, render_size, blend = ctx.args
        want_col = col is not None and ctx.needs_input_grad[1]
        g = grad_img.contiguous().float()
        grad_pts, grad_col = render_points_backward(pts, col, radius, render_size, blend, planes, g, want_col)
        return grad_pts, grad_col, None, None, None


def render_points(points, colors=None, radius=0.005, render_size=224, blend=None):
    """The library's renderer as a differentiable torch operation (genpc_render_points / genpc_render_points_backward,
    csrc/render_grad.hip): points [N,3] -> image [S,S,3], or [B,N,3] -> [B,S,S,3] (B clouds of equal size, one call); colors of
    the points' shape in [0,1], None = white.  The camera is the library's one (eye (0,0,3) looking at the origin, focal 4);
    radius is used as given (ObjectPoseOptim applies the reference's factor 1.1).
    blend: 1 Pulsar's blending function, 0 the coverage splat, None the calling thread's render_tune mode AT FORWARD TIME -- the
    backward uses the forward's blend whatever thread it runs on and whatever mode is set by then.
    Gradients go to `points`, and to `colors` when it requires grad (otherwise the colour gradient is not computed); none to
    the radius.  once_differentiable: no double backward.  The backward sums in a fixed order: the same bits in every run.
    GPU tensors only."""
    if not torch.is_tensor(points):
        raise TypeError("render_points: points must be a tensor")
    _lib.require_gpu(points)
    if points.dim() not in (2, 3) or points.shape[-1] != 3:
        raise ValueError("render_points: points must be [N,3] or [B,N,3], got %s" % (tuple(points.shape),))
    if colors is not None:
        if not torch.is_tensor(colors):
            colors = torch.as_tensor(colors, device=points.device)
        _lib.require_gpu(colors)
        if colors.shape != points.shape:
            raise ValueError("render_points: colors must have the shape of points %s, got %s" % (tuple(points.shape), tuple(colors.shape)))
    if blend is None:
        blend = _thread_blend()
    elif blend not in (0, 1):
        raise ValueError("render_points: blend must be None, 0 or 1, got %r" % (blend,))
    single = points.dim() == 2
    pts = (points[None] if single else points).float().contiguous()
    col = None if colors is None else (colors[None] if single else colors).float().contiguous()
    img = _RenderPoints.apply(pts, col, float(radius), int(render_size), int(blend))
    return img[0] if single else img


RENDER_RAGGED_MAX_ELEMENTS = 384          # genpc_hip.h GENPC_RENDER_RAGGED_MAX_ELEMENTS: clouds of one library call


def _host_floats(values):
    """(a ctypes float array of the values, its void pointer -- which keeps the array alive)"""
    arr = (ctypes.c_float * max(1, len(values)))(*[float(v) for v in values])
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def render_points_ragged_forward(pts, off, col, radii, render_size, blend):
    """genpc_render_points_ragged on packed clouds: pts [T,3] float32 GPU, off S + 1 host ints, col None (white) or [T,3], radii S
    host floats -> (img [S,size,size,3], planes [S,5,size*size]).  More than 384 clouds go in several library calls."""
    from .. import _ragged
    s, size = len(off) - 1, int(render_size)
    img = torch.empty(s, size, size, 3, device=pts.device)
    planes = torch.empty(s, 5, size * size, device=pts.device)
    for a, b, o in _ragged.chunks(RENDER_RAGGED_MAX_ELEMENTS, off):
        _, op = _ragged.host_ints(o, "offsets")
        _, rp = _host_floats(radii[a:b])
        rc = _lib.on_device_of(pts, _L.genpc_render_points_ragged, b - a, op, _p(pts[off[a]:off[b]]),
                               _p(None if col is None else col[off[a]:off[b]]), rp, size, int(blend), _p(img[a:b]), _p(planes[a:b]))
        if rc != 1:
            raise RuntimeError("genpc_render_points_ragged failed (rc=%d): %s" % (rc, _lib.last_error()))
    return img, planes


def render_points_ragged_backward(pts, off, col, radii, render_size, blend, planes, grad_img, want_col=True):
    """genpc_render_points_ragged_backward: planes as render_points_ragged_forward returned them for the same arguments, grad_img
    [S,size,size,3] -> (grad_pts [T,3], grad_col [T,3] or None)."""
    from .. import _ragged
    empty = pts.shape[0] == 0
    grad_pts = torch.zeros_like(pts) if empty else torch.empty_like(pts)
    grad_col = (torch.zeros_like(pts) if empty else torch.empty_like(pts)) if want_col else None
    for a, b, o in _ragged.chunks(RENDER_RAGGED_MAX_ELEMENTS, off):
        _, op = _ragged.host_ints(o, "offsets")
        _, rp = _host_floats(radii[a:b])
        rc = _lib.on_device_of(pts, _L.genpc_render_points_ragged_backward, b - a, op, _p(pts[off[a]:off[b]]),
                               _p(None if col is None else col[off[a]:off[b]]), rp, int(render_size), int(blend), _p(planes[a:b]),
                               _p(grad_img[a:b]), _p(grad_pts[off[a]:off[b]]), _p(None if grad_col is None else grad_col[off[a]:off[b]]))
        if rc != 1:
            raise RuntimeError("genpc_render_points_ragged_backward failed (rc=%d): %s" % (rc, _lib.last_error()))
    return grad_pts, grad_col


class _RenderPointsRagged(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts, col, off, radii, render_size, blend):
        img, planes = render_points_ragged_forward(pts, off, col, radii, render_size, blend)
        if col is None:
            ctx.save_for_backward(pts, planes)
        else:
            ctx.save_for_backward(pts, planes, col)
        ctx.args = (tuple(off), tuple(radii), int(render_size), int(blend))      # (the blend of the FORWARD, as in _RenderPoints)
        return img

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_img):
        saved = ctx.saved_tensors
        pts, planes, col = saved[0], saved[1], saved[2] if len(saved) > 2 else None
        off, radii, render_size, blend = ctx.args
        want_col = col is not None and ctx.needs_input_grad[1]
        g = grad_img.contiguous().float()
        grad_pts, grad_col = render_points_ragged_backward(pts, list(off), col, list(radii), render_size, blend, planes, g, want_col)
        return grad_pts, grad_col, None, None, None, None


def _per_element(value, s, fn, name):
    """a float, or S host floats -> a list of S Python floats"""
    if torch.is_tensor(value):
        value = value.detach().cpu().tolist()
    if hasattr(value, "tolist"):          # a numpy array or scalar
        value = value.tolist()
    if not isinstance(value, (str, bytes)) and hasattr(value, "__iter__"):
        vals = [float(v) for v in value]
        if len(vals) != s:
            raise ValueError("%s: %s must be a float or one float per cloud (%d), got %d" % (fn, name, s, len(vals)))
        return vals
    return [float(value)] * s


def camera_points(points, R, T, focal=4.0):
    """The affine map that takes world points seen by a pinhole camera (R [3,3], T [3], focal) in pytorch3d's convention --
    X_view = X R + T, +X left, +Y up, +Z into the scene -- into the library's camera frame, where the library's own camera draws
    what that camera sees once the radius is scaled by focal / 4:  with D = diag(-f/4, f/4, -1),
        p = X (R D) + (T D + (0, 0, 3)).
    R D and T D + (0,0,3) are formed first, then one affine map is applied as sums of products in a fixed order (no matrix
    kernel): the library's own camera (R = diag(-1, 1, -1), T = (0, 0, 3), f = 4) is the identity exactly, a signed-permutation R
    with T = (0, 0, 3) and a power-of-two focal maps without rounding.  points [...,3]; plain torch: gradients to points, R and T
    are autograd's; focal is a host float (it also enters through the radius, which has no gradient)."""
    if not torch.is_tensor(points) or points.shape[-1] != 3:
        raise ValueError("camera_points: points must be a [...,3] tensor")
    R = torch.as_tensor(R, dtype=points.dtype if not torch.is_tensor(R) else None).to(device=points.device, dtype=points.dtype)
    T = torch.as_tensor(T, dtype=points.dtype if not torch.is_tensor(T) else None).to(device=points.device, dtype=points.dtype)
    if tuple(R.shape) != (3, 3) or tuple(T.shape) != (3,):
        raise ValueError("camera_points: R must be [3,3] and T [3], got %s and %s" % (tuple(R.shape), tuple(T.shape)))
    f = float(focal)
    if not f > 0.0:
        raise ValueError("camera_points: focal must be positive, got %r" % (focal,))
    d = torch.tensor([-f / 4.0, f / 4.0, -1.0], dtype=points.dtype, device=points.device)
    M = R * d
    t = T * d + torch.tensor([0.0, 0.0, 3.0], dtype=points.dtype, device=points.device)
    return points[..., 0:1] * M[0] + points[..., 1:2] * M[1] + points[..., 2:3] * M[2] + t


def look_at_view_transform(eye, at=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """pytorch3d's look_at_view_transform for V eyes: eye [V,3] or [3] (at, up alike, or one for all) -> (R [V,3,3], T [V,3]),
    float32 on the CPU, with X_view = X R + T:  z = normalize(at - eye), x = normalize(up x z), y = z x x, R has x, y, z as
    COLUMNS and T = -eye R.  Formed in float64.  Eye (0,0,3) gives the library's camera: R = diag(-1, 1, -1), T = (0, 0, 3)."""
    e = torch.as_tensor(eye, dtype=torch.float64).reshape(-1, 3)
    a = torch.as_tensor(at, dtype=torch.float64).reshape(-1, 3).expand_as(e)
    u = torch.as_tensor(up, dtype=torch.float64).reshape(-1, 3).expand_as(e)
    z = torch.nn.functional.normalize(a - e, dim=-1)
    x = torch.nn.functional.normalize(torch.cross(u, z, dim=-1), dim=-1)
    y = torch.cross(z, x, dim=-1)
    if not bool(torch.isfinite(x).all()) or bool((x.norm(dim=-1) < 0.5).any()):
        raise ValueError("look_at_view_transform: up is parallel to the viewing direction (or eye == at)")
    R = torch.stack((x, y, z), dim=-1)
    T = -(e[:, None, :] @ R)[:, 0, :]
    return (R + 0.0).float(), (T + 0.0).float()          # (+ 0: no negative zeros)


def _camera_list(cameras, s, fn):
    """(R, T, focal) -> S triples (R_j [3,3], T_j [3], f_j)"""
    if not isinstance(cameras, (list, tuple)) or len(cameras) != 3:
        raise ValueError("%s: cameras must be None or (R, T, focal)" % fn)
    R, T, focal = cameras
    R, T = torch.as_tensor(R), torch.as_tensor(T)
    if tuple(R.shape) == (3, 3):
        R = R[None].expand(s, 3, 3)
    if tuple(T.shape) == (3,):
        T = T[None].expand(s, 3)
    if tuple(R.shape) != (s, 3, 3) or tuple(T.shape) != (s, 3):
        raise ValueError("%s: cameras' R must be [%d,3,3] or [3,3] and T [%d,3] or [3], got %s and %s" % (fn, s, s, tuple(R.shape), tuple(T.shape)))
    f = _per_element(focal, s, fn, "focal")
    for j, v in enumerate(f):
        if not v > 0.0:
            raise ValueError("%s: the focal of camera %d must be positive, got %r" % (fn, j, v))
    return [(R[j], T[j], f[j]) for j in range(s)]


def render_points_ragged(clouds, colors=None, radius=0.005, render_size=224, blend=None, cameras=None):
    """render_points for S clouds of DIFFERENT sizes in one call, each with its own radius and, if asked, its own camera
    (genpc_render_points_ragged / genpc_render_points_ragged_backward) -> [S,size,size,3].
    clouds: a list of [N_j,3] float32 GPU tensors or packed (points [T,3], offsets); a cloud may be empty (its image is the
    background).  colors: None (white) or the same form with the same sizes.  radius: a float or S host floats, used as given.
    blend: as in render_points -- None is the calling thread's render_tune mode AT FORWARD TIME, kept for the backward.
    cameras: None -- the library's camera, no map at all -- or (R, T, focal): R [S,3,3] or [3,3], T [S,3] or [3], focal a float
    or S host floats, pytorch3d's convention (camera_points).  Cloud j is mapped by camera_points in plain torch and drawn with
    radius_j focal_j / 4; znear, zfar and gamma stay the library's.
    Image j is bit for bit render_points of cloud j alone (mapped, with its radius).  Gradients go to every list element (or to
    the packed points), to the colours when they require grad (otherwise the colour gradient is not computed), through the map
    to R and T; none to the radius or the focal.  once_differentiable.  More than 384 clouds go in several library calls."""
    from .. import _ragged
    fn = "render_points_ragged"
    pts, off = _ragged.ragged_side(clouds, fn, "clouds")
    s = len(off) - 1
    if s == 0:
        raise ValueError("%s: clouds is empty" % fn)
    _lib.require_gpu(pts)
    col = None
    if colors is not None:
        col, coff = _ragged.ragged_side(colors, fn, "colors")
        if coff != off:
            raise ValueError("%s: colors must have the sizes of clouds" % fn)
        _lib.require_gpu(col)
    if blend is None:
        blend = _thread_blend()
    elif blend not in (0, 1):
        raise ValueError("%s: blend must be None, 0 or 1, got %r" % (fn, blend))
    radii = _per_element(radius, s, fn, "radius")
    if cameras is not None:
        cams = _camera_list(cameras, s, fn)
        pts = torch.cat([camera_points(pts[off[j]:off[j + 1]], *cams[j]) for j in range(s)], dim=0).contiguous()
        radii = [radii[j] * (cams[j][2] / 4.0) for j in range(s)]
    for j, r in enumerate(radii):
        if not r > 0.0:
            raise ValueError("%s: the radius of cloud %d must be positive, got %r" % (fn, j, r))
    return _RenderPointsRagged.apply(pts, col, off, radii, int(render_size), int(blend))


def rotation_6d_to_matrix(d6):
    """Zhou et al.'s 6-D rotation (CVPR 2019), pytorch3d's convention: Gram-Schmidt of the two 3-vectors, the three results as
    ROWS.  [...,6] -> [...,3,3]."""
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = torch.nn.functional.normalize(a1, dim=-1)
    b2 = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = torch.nn.functional.normalize(b2, dim=-1)
    b3 = torch.cross(b1, b2, dim=-1)
    return torch.stack((b1, b2, b3), dim=-2)


def matrix_to_rotation_6d(matrix):
    """the first two rows of [...,3,3] as [...,6] (the inverse of rotation_6d_to_matrix on rotations)"""
    return matrix[..., :2, :].clone().reshape(matrix.shape[:-2] + (6,))


def get_init_rot(axis, angle_deg, device):
    """diff_obj_pose.py:470-493: the 6-D form of the rotation by angle_deg degrees about `axis` ('x', 'y', 'z' or a 3-vector,
    normalised here) -> [6] float32 on device.  Rodrigues' formula R = I + sin t K + (1 - cos t) K^2."""
    if isinstance(axis, str):
        names = {"x": (1.0, 0.0, 0.0), "y": (0.0, 1.0, 0.0), "z": (0.0, 0.0, 1.0)}
        if axis.lower() not in names:
            raise ValueError("unknown axis %r: 'x', 'y', 'z' or a 3-vector" % (axis,))
        k = torch.tensor(names[axis.lower()], dtype=torch.float32)
    else:
        k = torch.as_tensor(axis, dtype=torch.float32).reshape(-1).cpu()
        if k.numel() != 3:
            raise ValueError("a custom axis must have 3 entries")
        k = k / (k.norm() + 1e-8)
    t = math.radians(angle_deg)
    K = torch.tensor([[0.0, -float(k[2]), float(k[1])], [float(k[2]), 0.0, -float(k[0])], [-float(k[1]), float(k[0]), 0.0]], dtype=torch.float64)
    R = torch.eye(3, dtype=torch.float64) + math.sin(t) * K + (1.0 - math.cos(t)) * (K @ K)
    return matrix_to_rotation_6d(R.float()[None])[0].to(device)


def build_transform(R_obj, t, scale):
    """diff_obj_pose.py:464-468: [[s R, t], [0, 1]]"""
    T = torch.eye(4, device=R_obj.device)
    T[:3, :3] = R_obj * scale
    T[:3, 3] = t
    return T


def _luminance(img):
    return 0.299 * img[:, :, 0] + 0.587 * img[:, :, 1] + 0.114 * img[:, :, 2]


def normalize_images(ref_img, result_img, method="statistical"):
    """diff_obj_pose.py:201-236: result_img's per-channel mean and (unbiased) std moved onto ref_img's, clamped to [0,1];
    'histogram': the same with the luminances' scalar statistics; anything else: unchanged.  -> (ref_img, result_normalized)"""
    if method == "statistical":
        ref_mean = torch.mean(ref_img, dim=(0, 1), keepdim=True)
        ref_std = torch.std(ref_img, dim=(0, 1), keepdim=True) + 1e-6
        res_mean = torch.mean(result_img, dim=(0, 1), keepdim=True)
        res_std = torch.std(result_img, dim=(0, 1), keepdim=True) + 1e-6
    elif method == "histogram":
        rg, sg = _luminance(ref_img), _luminance(result_img)
        ref_mean, ref_std = torch.mean(rg), torch.std(rg) + 1e-6
        res_mean, res_std = torch.mean(sg), torch.std(sg) + 1e-6
    else:
        return ref_img, result_img
    return ref_img, torch.clamp((result_img - res_mean) / res_std * ref_std + ref_mean, 0.0, 1.0)


def compute_soft_mask(rendered_img, threshold=0.1, tau=0.05, method="luminance"):
    """diff_obj_pose.py:258-275: sigmoid((occupancy - threshold) / tau), occupancy the luminance or ('occupancy') the channel sum"""
    occ = rendered_img.sum(-1) if method == "occupancy" else _luminance(rendered_img)
    return torch.sigmoid((occ - threshold) / tau)


def dice_loss(pred_mask, target_mask, smooth=1e-6):
    """diff_obj_pose.py:239-256: 1 - (2 sum(p t) + smooth) / (sum p + sum t + smooth)"""
    p, t = pred_mask.reshape(-1), target_mask.reshape(-1)
    return 1 - (2.0 * (p * t).sum() + smooth) / (p.sum() + t.sum() + smooth)


def soft_iou_loss(result_img, ref_mask, threshold=0.1, tau=0.05, method="luminance", smooth=1e-6):
    """diff_obj_pose.py:181-199 -> (1 - iou, iou, the soft mask of result_img)"""
    pred = compute_soft_mask(result_img, threshold, tau, method)
    inter = (pred * ref_mask).sum()
    union = pred.sum() + ref_mask.sum() - inter
    iou = (inter + smooth) / (union + smooth)
    return 1.0 - iou, iou, pred


def edge_loss(ref_img, result):
    """diff_obj_pose.py:277-284: MSE between the absolute differences of neighbouring pixels, along both image axes"""
    mse = torch.nn.functional.mse_loss
    eh = lambda x: torch.abs(x[:, :-1, :] - x[:, 1:, :])
    ev = lambda x: torch.abs(x[:-1, :, :] - x[1:, :, :])
    return mse(eh(ref_img), eh(result)) + mse(ev(ref_img), ev(result))


LOSS_WEIGHTS = dict(mse=0.0, edge=0.0, mask=1.0, iou=0.0, cd=3.0)      # diff_obj_pose.py:329-334


def _loss_weights(weights):
    w = dict(LOSS_WEIGHTS)
    if weights is None:
        return w
    if isinstance(weights, dict):
        unknown = set(weights) - set(w)
        if unknown:
            raise ValueError("compute_loss_function: unknown weights %s (known: %s)" % (sorted(unknown), sorted(w)))
        w.update({k: float(v) for k, v in weights.items()})
        return w
    vals = [float(v) for v in weights]
    if len(vals) != 5:
        raise ValueError("compute_loss_function: weights is a dict or the five numbers (mse, edge, mask, iou, cd)")
    return dict(zip(("mse", "edge", "mask", "iou", "cd"), vals))


def compute_loss_function(ref_img, result, ref_mask=None, ref_points=None, result_points=None, cdloss=None, weights=None):
    """diff_obj_pose.py:286-336 -> (total_loss, mse_loss, edge_loss_value, iou_loss_value, iou_value, cd_loss_value, mask_loss):
    the images statistically normalised, their soft masks, mask_loss = 30 MSE + BCE + 10 Dice of the masks, the soft IoU against
    ref_mask (when given), cd = partial_l1(result_points, ref_points) + 0.5 partial_l1(ref_points, result_points) (when both are
    given; cdloss: a Completionloss, made here when None).
    weights: None = the reference's (mse 0, edge 0, mask 1, iou 0, cd 3); a dict over those names or the five numbers in that
    order -- the reference's comment invites the edit.  A term whose weight is 0 is still returned, as in the reference; the
    edge term, which the reference leaves commented out and returns as 0, is evaluated when its weight is not 0."""
    F = torch.nn.functional
    w = _loss_weights(weights)
    ref_n, res_n = normalize_images(ref_img, result)
    mask_result, mask_ref = compute_soft_mask(res_n, 0.1, 0.05), compute_soft_mask(ref_n, 0.1, 0.05)
    mse_loss = F.mse_loss(ref_n, res_n)
    mask_loss = F.mse_loss(mask_result, mask_ref) * 30 + F.binary_cross_entropy(mask_result, mask_ref)
    mask_loss = mask_loss * 1 + dice_loss(mask_result, mask_ref) * 10
    zero = lambda v=0.0: torch.tensor(v, device=result.device)
    edge_loss_value = edge_loss(ref_n, res_n) if w["edge"] != 0.0 else zero()
    iou_loss_value, iou_value = zero(), zero(1.0)
    if ref_mask is not None:
        iou_loss_value, iou_value, _ = soft_iou_loss(res_n, ref_mask, threshold=0.1, tau=0.05)
    cd_loss_value = zero()
    if ref_points is not None and result_points is not None:
        if cdloss is None:
            from ..utils.loss_util import Completionloss
            cdloss = Completionloss(loss_func="cd_l1")
        cd_loss_value = cdloss.chamfer_partial_l1(result_points.unsqueeze(0), ref_points.unsqueeze(0)) + \
            0.5 * cdloss.chamfer_partial_l1(ref_points.unsqueeze(0), result_points.unsqueeze(0))
    total_loss = mse_loss * w["mse"] + edge_loss_value * w["edge"] + mask_loss * w["mask"] + iou_loss_value * w["iou"] + cd_loss_value * w["cd"]
    return total_loss, mse_loss, edge_loss_value, iou_loss_value, iou_value, cd_loss_value, mask_loss


# the library's one camera in pytorch3d's look_at_view_transform form (eye (0,0,3), at the origin, up +y): X_view = X_world R + T
_CAMERA_R = ((-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, -1.0))
_CAMERA_T = (0.0, 0.0, 3.0)
_CAMERA_FOCAL = 4.0
_CAMERA_WORDS = "the library has one camera: eye (0,0,3) looking at the origin, up +y (R = diag(-1, 1, -1), T = (0, 0, 3)), focal 4.0"


def render_reference_image(vert_pos, vert_col, radius, render_size, device):
    """diff_obj_pose.py:108-134: the partial cloud's image under the fixed camera -> (ref_img [S,S,3], ref_mask [S,S],
    R_cam [1,3,3], T_cam [1,3]); vert_col None = white.  No gradient is recorded."""
    with torch.no_grad():
        pts = torch.as_tensor(vert_pos, dtype=torch.float32, device=device)
        col = None if vert_col is None else torch.as_tensor(vert_col, dtype=torch.float32, device=device)
        result = render_points(pts, col, radius, render_size)
    R = torch.tensor([_CAMERA_R], dtype=torch.float32, device=device)
    T = torch.tensor([_CAMERA_T], dtype=torch.float32, device=device)
    return result, compute_mask_from_rendering(result), R, T


class ObjectPoseOptim(nn.Module):
    """diff_obj_pose.py:339-436: the 7-DoF pose (6-D rotation, translation, log scale) of a cloud as an nn.Module whose forward
    poses the cloud in plain torch and renders it with render_points at 1.1 x radius.  Parameters rot_6d [6], trans [3],
    log_scale [1] (log 0.75); buffer center (the cloud's mean).  vert_col None = white.  R_cam / T_cam / focal must describe the
    library's one camera (what render_reference_image returns); another camera or focal raises ValueError.
    project_every > 0: every that many forwards rot_6d is replaced by the 6-D form of the nearest rotation."""

    def __init__(self, vert_pos, vert_col, radius, render_size, device, R_cam, T_cam, init_rot, focal=4.0, project_every=0):
        super().__init__()
        Rc = torch.as_tensor(R_cam, dtype=torch.float32).reshape(-1).cpu()
        Tc = torch.as_tensor(T_cam, dtype=torch.float32).reshape(-1).cpu()
        if Rc.numel() != 9 or Tc.numel() != 3 or not torch.allclose(Rc, torch.tensor(_CAMERA_R).reshape(-1), atol=1e-6) \
                or not torch.allclose(Tc, torch.tensor(_CAMERA_T), atol=1e-6):
            raise ValueError("ObjectPoseOptim: unsupported camera R_cam / T_cam; " + _CAMERA_WORDS)
        if float(focal) != _CAMERA_FOCAL:
            raise ValueError("ObjectPoseOptim: unsupported focal %r; %s" % (focal, _CAMERA_WORDS))
        self.device = device
        self.render_size = int(render_size)
        self.radius = float(radius)
        self.gamma = 1e-2
        self.project_every = project_every
        vert_pos = torch.as_tensor(vert_pos, dtype=torch.float32, device=device)
        self.register_parameter("vert_pos", nn.Parameter(vert_pos, requires_grad=False))
        if vert_col is None:
            self.vert_col = None
        else:
            self.register_parameter("vert_col", nn.Parameter(torch.as_tensor(vert_col, dtype=torch.float32, device=device), requires_grad=False))
        self.register_buffer("center", vert_pos.mean(0))
        self.rot_6d = nn.Parameter(torch.as_tensor(init_rot, dtype=torch.float32, device=device).clone())
        self.trans = nn.Parameter(torch.zeros(3, dtype=torch.float32, device=device))
        self.log_scale = nn.Parameter(torch.tensor([math.log(0.75)], dtype=torch.float32, device=device))
        self.register_buffer("R_cam", torch.as_tensor(R_cam, dtype=torch.float32, device=device))
        self.register_buffer("T_cam", torch.as_tensor(T_cam, dtype=torch.float32, device=device))
        self.register_buffer("focal_length", torch.tensor([float(focal)], dtype=torch.float32, device=device))
        self._step = 0

    def get_current_RT(self):
        R = rotation_6d_to_matrix(self.rot_6d[None])[0].detach()
        return R, self.trans.detach(), torch.exp(self.log_scale.detach())[0]

    def get_transform(self):
        R, t, s = self.get_current_RT()
        return build_transform(R, t, s)

    @staticmethod
    def _project_to_rotation(R):
        U, _, Vh = torch.linalg.svd(R.double())
        d = torch.sign(torch.linalg.det(U @ Vh))
        D = torch.diag(torch.stack([torch.ones_like(d), torch.ones_like(d), d]))
        return (U @ D @ Vh).to(R.dtype)

    def forward(self, return_pts=False, project_now=False):
        if project_now or (self.project_every > 0 and self._step % self.project_every == 0 and self._step > 0):
            with torch.no_grad():
                R_proj = self._project_to_rotation(rotation_6d_to_matrix(self.rot_6d[None])[0])
                self.rot_6d.data = matrix_to_rotation_6d(R_proj[None])[0].data
        self._step += 1
        R_obj = rotation_6d_to_matrix(self.rot_6d[None])[0]
        scale = torch.exp(self.log_scale)[0]
        local = (self.vert_pos - self.center) * scale
        local = (R_obj @ local.T).T
        pts = local + self.center + self.trans
        img = self._render(pts)
        if return_pts:
            return img, R_obj, scale, pts
        return img, R_obj, scale

    def _render(self, pts):
        return render_points(pts, self.vert_col, 1.1 * self.radius, self.render_size)


def render_reference_images(vert_pos, vert_col, radius, render_size, R_cams, T_cams, focal=4.0):
    """render_reference_image under V cameras: vert_pos [N,3] (a float32 GPU tensor), vert_col None = white, R_cams [V,3,3],
    T_cams [V,3] (look_at_view_transform's form), focal a float or V floats -> (ref_imgs [V,S,S,3], ref_masks [V,S,S]).  One ragged
    call of V mapped copies; no gradient is recorded.  With the library's camera view v is render_reference_image's image."""
    with torch.no_grad():
        pts = torch.as_tensor(vert_pos).float()
        _lib.require_gpu(pts)
        col = None if vert_col is None else torch.as_tensor(vert_col, dtype=torch.float32, device=pts.device)
        v = int(torch.as_tensor(R_cams).reshape(-1, 3, 3).shape[0])
        imgs = render_points_ragged([pts] * v, None if col is None else [col] * v, radius, render_size,
                                    cameras=(torch.as_tensor(R_cams).reshape(-1, 3, 3), torch.as_tensor(T_cams).reshape(-1, 3), focal))
        masks = torch.stack([compute_mask_from_rendering(imgs[k]) for k in range(v)])
    return imgs, masks


class ObjectPoseOptimViews(ObjectPoseOptim):
    """ObjectPoseOptim under V cameras: the same parameters (rot_6d, trans, log_scale), buffers and pose statements; R_cams
    [V,3,3], T_cams [V,3] (look_at_view_transform's form), focal a float or V floats.  forward() returns (imgs [V,S,S,3], R_obj,
    scale[, pts]): the ONE posed cloud through render_points_ragged with V mapped copies at 1.1 x radius.  With the single
    library camera its image is ObjectPoseOptim's, bit for bit."""

    def __init__(self, vert_pos, vert_col, radius, render_size, device, R_cams, T_cams, init_rot, focal=4.0, project_every=0):
        super().__init__(vert_pos, vert_col, radius, render_size, device, [_CAMERA_R], [_CAMERA_T], init_rot, _CAMERA_FOCAL, project_every)
        R = torch.as_tensor(R_cams, dtype=torch.float32).reshape(-1, 3, 3)
        T = torch.as_tensor(T_cams, dtype=torch.float32).reshape(-1, 3)
        if R.shape[0] < 1 or T.shape[0] != R.shape[0]:
            raise ValueError("ObjectPoseOptimViews: R_cams must be [V,3,3] and T_cams [V,3], got %s and %s" % (tuple(R.shape), tuple(T.shape)))
        self.views = int(R.shape[0])
        self.focals = _per_element(focal, self.views, "ObjectPoseOptimViews", "focal")
        self.R_cam = R.to(device)
        self.T_cam = T.to(device)
        self.focal_length = torch.tensor(self.focals, dtype=torch.float32, device=device)

    def _render(self, pts):
        v = self.views
        return render_points_ragged([pts] * v, None if self.vert_col is None else [self.vert_col] * v, 1.1 * self.radius, self.render_size,
                                    cameras=(self.R_cam, self.T_cam, self.focals))


def object_pose_optimization_torch(complete_xyz, partial_xyz, radius=0.005, lr=0.005, iters=300, render_size=224, cam_bias_num=4,
                                   complete_col=None, partial_col=None, weights=None, loss_fn=None, return_history=False):
    """The reference's loop (diff_obj_pose.py:496-594) in torch on render_points -- the customisable path; object_pose_optimization
    is the fast one (a fused loop of the one default objective) and gives the same histories to the rounding of their sums.
    complete_xyz [Nc,3], partial_xyz [Np,3] GPU tensors with colours complete_col / partial_col (None = white).  Per start
    (rotated by 90 degrees about y each): ObjectPoseOptim under torch.optim.Adam with the groups rot_6d lr, trans 0.2 lr,
    log_scale 0.1 lr; iters + 1 steps of
        loss = compute_loss_function(ref_img, result, ref_mask, partial_xyz, pts, cdloss, weights)[0] + 0.001 |R R^T - I|_F
    or, with loss_fn, loss = loss_fn(ref_img, result, ref_mask, partial_xyz, pts, R_obj) (a scalar tensor: the whole objective).
    A start stops after 300 steps without a new best loss; the start with the lowest best loss gives the result, with the
    parameters it ENDED on (as in the reference).  Returns the 4x4 numpy [[sR, t], [0, 1]]; return_history: also the
    [cam_bias_num, iters + 1] losses (a start that stopped early repeats its last loss) and the [10] parameters."""
    import numpy as np
    from ..utils.loss_util import Completionloss
    complete_xyz = complete_xyz.contiguous().float()
    partial_xyz = partial_xyz.contiguous().float()
    _lib.check_tensors((("complete_xyz", complete_xyz), ("partial_xyz", partial_xyz)))
    if complete_xyz.dim() != 2 or partial_xyz.dim() != 2:
        raise ValueError("object_pose_optimization_torch: clouds must be [N,3], got %s and %s" % (tuple(complete_xyz.shape), tuple(partial_xyz.shape)))
    device = complete_xyz.device
    cc, pc = _col(complete_col, complete_xyz, "complete_col"), _col(partial_col, partial_xyz, "partial_col")
    cdloss = Completionloss(loss_func="cd_l1")
    ref_img, ref_mask, R_cam, T_cam = render_reference_image(partial_xyz, pc, radius, render_size, device)
    eye = torch.eye(3, device=device)
    hist = np.zeros((int(cam_bias_num), int(iters) + 1), np.float32)
    best_loss, best_state = float("inf"), None
    for start in range(int(cam_bias_num)):
        model = ObjectPoseOptim(complete_xyz, cc, radius, render_size, device, R_cam, T_cam, get_init_rot("y", start * 90, device))
        optimizer = torch.optim.Adam([{"params": [model.rot_6d], "lr": lr}, {"params": [model.trans], "lr": lr * 0.2},
                                      {"params": [model.log_scale], "lr": lr * 0.1}])
        patience, patience_counter, local_best, cur_loss = 300, 0, float("inf"), float("nan")
        for i in range(int(iters) + 1):
            optimizer.zero_grad()
            result, R_obj, scale, pts = model(return_pts=True)
            if loss_fn is not None:
                loss = loss_fn(ref_img, result, ref_mask, partial_xyz, pts, R_obj)
            else:
                total = compute_loss_function(ref_img, result, ref_mask, partial_xyz, pts, cdloss, weights)[0]
                loss = total + 0.001 * torch.norm(R_obj @ R_obj.T - eye)
            loss.backward()
            optimizer.step()
            cur_loss = loss.item()
            hist[start, i:] = cur_loss
            if cur_loss < local_best:
                local_best, patience_counter = cur_loss, 0
            else:
                patience_counter += 1
            if patience_counter > patience:
                break
        if local_best < best_loss:
            best_loss = local_best
            best_state = (model.rot_6d.detach().clone(), model.trans.detach().clone(), model.log_scale.detach().clone())
    if best_state is None:
        raise RuntimeError("object_pose_optimization_torch: no start gave a finite loss")
    rot_6d, trans, log_scale = best_state
    T_final = build_transform(rotation_6d_to_matrix(rot_6d[None])[0], trans, torch.exp(log_scale)[0])
    final_transform = T_final.detach().cpu().numpy()
    if return_history:
        return final_transform, hist, torch.cat([rot_6d, trans, log_scale]).cpu().numpy()
    return final_transform
