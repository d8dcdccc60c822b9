"""``emd_raggedDist`` / ``emd_raggedFunction``: the auction EMD of ``emdModule`` for c pairs of clouds of DIFFERENT sizes in one
library call (genpc_emd_forward_ragged, csrc/emd_ragged.hip).  The reference has no such call -- ``emdModule`` takes one n
for the whole batch -- so there is nothing of its interface to keep; per pair the results are those of ``emdModule`` on that
pair alone, bit for bit.  The auction needs equal sizes INSIDE a pair: clouds1[j] and clouds2[j] both have N_j points,
N_j % 256 == 0 (or 0).  Inputs follow dist_chamfer_ragged.py: lists of [N_j,3] float32 GPU tensors, or packed as
(points [T,3], offsets).  Gradient flows to the first clouds only (emd_module.py:83-87).
"""
import torch
from torch import nn
from torch.autograd import Function

from ... import _lib, emd
from ..._ragged import chunks, is_packed, pack_clouds


def check_pairs(off1, off2, who="emd_ragged"):
    """Both sides' offsets (c + 1 Python ints each) describe c pairs the auction can take; ValueError names the first that is not."""
    if len(off1) != len(off2):
        raise ValueError("%s: %d clouds against %d" % (who, len(off1) - 1, len(off2) - 1))
    for j in range(len(off1) - 1):
        n, m = off1[j + 1] - off1[j], off2[j + 1] - off2[j]
        if n != m:
            raise ValueError("%s: pair %d has %d points against %d (the auction needs equal sizes inside a pair)" % (who, j, n, m))
        if n % 256 != 0:
            raise ValueError("%s: pair %d has %d points, not a multiple of 256" % (who, j, n))


def alloc_state_ragged(total, device):
    """The eight state arrays of a ragged call, [total] each and UNINITIALISED: the call's first launch writes the initial
    state (loss_functions/emd/emd_module.py alloc_state's values).  Views of one allocation, 256-byte aligned."""
    pad = (total + 63) // 64 * 64
    names = ("dist", "price", "bid_increments", "max_increments", "assignment", "assignment_inv", "bid", "max_idx")
    block = torch.empty((len(names) * pad,), dtype=torch.int32, device=device)
    out = {name: block[k * pad:k * pad + total] for k, name in enumerate(names)}
    for name in names[:4]:
        out[name] = out[name].view(torch.float32)
    return out


def forward_packed(p1, p2, off, eps, iters):
    """Packed points [T,3] twice (float32, contiguous, one device) and the pairs' offsets -> the state arrays of the call(s):
    at most emd.RAGGED_MAX_PAIRS pairs per library call, a longer list takes several."""
    s = alloc_state_ragged(p1.shape[0], p1.device)
    for a, b, oa in chunks(emd.RAGGED_MAX_PAIRS, off):
        t0, t1 = off[a], off[b]
        rc = emd.forward_ragged(p1[t0:t1], p2[t0:t1], oa, s["dist"][t0:t1], s["assignment"][t0:t1],
                                s["price"][t0:t1], s["assignment_inv"][t0:t1], s["bid"][t0:t1], s["bid_increments"][t0:t1],
                                s["max_increments"][t0:t1], s["max_idx"][t0:t1], eps, iters)
        if rc == -1:
            raise ValueError("emd.forward_ragged refused the call: " + _lib.last_error())
        if rc != 1:
            raise RuntimeError("emd.forward_ragged failed: " + _lib.last_error())
    return s


class emd_raggedFunction(Function):
    """Packed points [T,3] twice (float32, contiguous, one device) and the pairs' host offsets (c + 1 Python ints, checked by
    the caller: emd_raggedDist does) -> dist [T], assignment [T] int32 (inside the pair's own second cloud, not
    differentiable); differentiable in the first points."""

    @staticmethod
    def forward(ctx, p1, p2, off, eps, iters):
        s = forward_packed(p1, p2, off, eps, iters)
        ctx.save_for_backward(p1, p2, s["assignment"])
        ctx.offsets = list(off)
        ctx.mark_non_differentiable(s["assignment"])
        return s["dist"], s["assignment"]

    @staticmethod
    def backward(ctx, graddist, gradidx):
        p1, p2, assignment = ctx.saved_tensors
        off = ctx.offsets
        graddist = graddist.contiguous()
        gradxyz1 = torch.zeros_like(p1)
        gradxyz2 = torch.zeros_like(p2)
        for a, b, oa in chunks(emd.RAGGED_MAX_PAIRS, off):
            t0, t1 = off[a], off[b]
            rc = emd.backward_ragged(p1[t0:t1], p2[t0:t1], oa, gradxyz1[t0:t1], graddist[t0:t1], assignment[t0:t1])
            if rc != 1:
                raise RuntimeError("emd.backward_ragged failed: " + _lib.last_error())
        return gradxyz1, gradxyz2, None, None, None


class emd_raggedDist(nn.Module):
    """forward(clouds1, clouds2, eps, iters): clouds as lists of [N_j,3] float32 GPU tensors or as (points, offsets), pair j
    of N_j points on both sides.  Returns (dist, assignment) in the form the first input came in: a list of [N_j] tensors per
    pair for a list, packed [T] tensors for a packed input.  dist carries the gradient to every element of the first list
    (through torch.cat), or to the packed points; the second clouds get zeros."""

    def __init__(self):
        super(emd_raggedDist, self).__init__()

    def forward(self, clouds1, clouds2, eps, iters):
        packed = is_packed(clouds1)
        p1, off1 = pack_clouds(clouds1, "clouds1")
        p2, off2 = pack_clouds(clouds2, "clouds2")
        check_pairs(off1, off2, "emd_raggedDist")
        _lib.require_gpu(p1, p2)
        if p1.device != p2.device:
            raise ValueError("emd_raggedDist: clouds1 and clouds2 are on different devices")
        dist, assignment = emd_raggedFunction.apply(p1, p2, off1, eps, iters)
        if packed:
            return dist, assignment
        sizes = [b - a for a, b in zip(off1, off1[1:])]
        return list(torch.split(dist, sizes)), list(torch.split(assignment, sizes))
