"""Farthest point sampling on the gfx950 library: the deterministic counterpart of
``fpsample.fps_sampling(points, k)`` as the reference calls it (main.py:21-24,
reg_xyz.py:215, DepthPrompting.py:88).  Start index 0 (fpsample starts at a random
index, so the reference's own subsamples are not reproducible)."""
import threading as _threading

import torch

from . import _lib

_L = _lib.lib
_p = _lib.ptr
# what the device-side verification has seen in this process (tools/soak_lanes.py prints it): clouds sampled, clouds whose
# hand-off timed out (first index -1) or whose sequence failed the check -- a step's sample was not the first arg-max
# (first index -2) -- and were sampled again
stats = {"clouds": 0, "timed_out": 0, "failed_check": 0}
MAX_POINTS = 4194304          # csrc/fps_plan.h: kFpsLargeMaxN
_stats_lock = _threading.Lock()


def fps_sampling(points, k):
    """points: [N,3] or [C,N,3] GPU tensor -> int32 indices [k] or [C,k], N up to 4194304.  The first
    index is always 0; the kernel writes -1 there if its inter-workgroup hand-off timed
    out (another kernel kept the cloud's workgroups from being co-resident).  Which of the
    library's three samplers a cloud takes follows from N alone (csrc/fps_plan.h); all return
    the same sequence."""
    single = points.dim() == 2
    pts = (points[None] if single else points).contiguous().float()
    _lib.check_tensors((("points", pts),))
    c, n, _ = pts.shape
    out = torch.empty(c, k, device=pts.device, dtype=torch.int32)
    rc = _lib.on_device_of(pts, _L.genpc_fps, c, n, _p(pts), int(k), _p(out))
    if rc == -1:
        raise ValueError("fps_sampling: need 0 < k <= N <= %d (k=%d, N=%d)" % (MAX_POINTS, k, n))
    if rc != 1:
        raise RuntimeError("genpc_fps failed: " + _lib.last_error())
    # index 0 is the start point of every cloud; the kernel writes -1 there when a hand-off
    # between its workgroups timed out (the samples after it would be garbage): those clouds go again, one at a time
    first = out[:, 0].tolist()
    bad = [j for j, f in enumerate(first) if f != 0]
    if bad:
        # (counted as _fps_multi_direct counts them: a failed check is visible whichever form was called)
        with _stats_lock:
            stats["timed_out"] += sum(1 for j in bad if first[j] != -2)
            stats["failed_check"] += sum(1 for j in bad if first[j] == -2)
    for j in bad:
        out[j] = _fps_multi_direct([pts[j]], [k])[0]
    return out[0] if single else out


def fps_sampling_multi(clouds, ks):
    """Several clouds of different sizes / sample counts in ONE pass (FPS is latency-bound: k sequential
    steps per cloud, so independent clouds side by side cost the longest one, not the sum).
    clouds: list of [N_j,3] GPU tensors, ks: list of ints -> list of int32 index tensors [k_j]."""
    return _fps_multi_direct(clouds, ks)


def fps_sampling_large(clouds, ks):
    """fps_sampling_multi with every cloud on the sampler that clouds beyond 262144 points take (csrc/fps_large.hip: one
    workgroup per cloud, its state in global memory, nothing that has to be co-resident), whatever its size.  Same sequences."""
    return _fps_multi_direct(clouds, ks, _entry="genpc_fps_large")


def _fps_multi_direct(clouds, ks, _attempt=0, _entry="genpc_fps_multi"):
    import ctypes
    pts = [c.contiguous().float() for c in clouds]
    _lib.check_tensors(tuple(("clouds[%d]" % j, p) for j, p in enumerate(pts)))
    c = len(pts)
    if c == 0:
        return []
    if len(ks) != c or any(p.dim() != 2 or p.shape[1] != 3 for p in pts):
        raise ValueError("fps_sampling_multi: need one k per [N,3] cloud")
    dev = pts[0].device
    outs = [torch.empty(int(k), device=dev, dtype=torch.int32) for k in ks]
    n_arr = (ctypes.c_int * c)(*[int(p.shape[0]) for p in pts])
    k_arr = (ctypes.c_int * c)(*[int(k) for k in ks])
    x_arr = (ctypes.c_void_p * c)(*[p.data_ptr() for p in pts])
    o_arr = (ctypes.c_void_p * c)(*[o.data_ptr() for o in outs])
    rc = _lib.on_device_of(pts[0], getattr(_L, _entry), c, ctypes.addressof(n_arr), ctypes.addressof(k_arr),
                           ctypes.addressof(x_arr), ctypes.addressof(o_arr))
    if rc == -1:
        raise ValueError("fps_sampling_multi: need 0 < k <= N <= %d for every cloud" % MAX_POINTS)
    if rc != 1:
        raise RuntimeError(_entry + " failed: " + _lib.last_error())
    first = torch.stack([o[0] for o in outs]).tolist()          # (one host read for all clouds)
    bad = [j for j, f in enumerate(first) if f != 0]
    with _stats_lock:
        stats["clouds"] += c if _attempt == 0 else 0
        stats["timed_out"] += sum(1 for j in bad if first[j] != -2)
        stats["failed_check"] += sum(1 for j in bad if first[j] == -2)
    if bad and (c > 1 or _attempt < 3):
        # out[0] == -1: a hand-off timed out (something else on the GPU kept a cloud's workgroups from running together), or
        # the device-side verification (csrc/fps_verify.hip: fps_verify_kernel) found a step whose sample is not the first arg-max --
        # seen twice for samplings running beside other streams' kernels, cause unknown.  Not an error yet: the clouds that
        # failed go again, one at a time (a launch to itself needs a fraction of the device)
        for j in bad:
            outs[j] = _fps_multi_direct([pts[j]], [ks[j]], _attempt=_attempt + 1 if c == 1 else _attempt, _entry=_entry)[0]
        return outs
    if bad:
        raise RuntimeError("genpc_fps: no verified sampling after %d attempts (hand-off timed out or the sequence failed its "
                           "device-side check every time)" % (_attempt + 1))
    return outs


def fps_subsample(points, k):
    """The helper metric.py calls but never defines: [B,N,3] -> [B,k,3]."""
    idx = fps_sampling(points, k).long()
    if points.dim() == 2:
        return points[idx]
    return torch.gather(points, 1, idx[..., None].expand(-1, -1, 3))
