"""``chamfer_ragged``: both Chamfer directions for clouds of different sizes in one call per direction
(genpc_nm_distance_ragged).  The reference never batches unequal clouds -- it scores one file at a time (metric.py:10-48)
-- so there is nothing of its interface to keep here; the results per pair are those of ``chamfer_3DDist`` on that pair
alone.  ``chamfer_ragged`` is forward only; ``chamfer_raggedDist`` / ``chamfer_raggedFunction`` are the same distances as a
loss: their backward is genpc_chamfer_backward_ragged, whose gradient rows are summed in a fixed order (the same bits on
every run, unlike ``chamfer_3DDist``'s atomics).
"""
import torch
from torch import nn
from torch.autograd import Function

from ... import _lib, chamfer_3D
from ..._ragged import _is_offsets, chunks, pack_clouds          # (both names are read from here too)


def _one_way(q, qoff, t, toff, search=None):
    """Queries against targets, at most chamfer_3D.RAGGED_MAX_PAIRS pairs per library call (a longer list takes several)."""
    dist = torch.empty((q.shape[0],), dtype=torch.float32, device=q.device)
    idx = torch.empty((q.shape[0],), dtype=torch.int32, device=q.device)
    for a, b, qa, ta in chunks(chamfer_3D.RAGGED_MAX_PAIRS, qoff, toff):
        q0, q1, t0, t1 = qoff[a], qoff[b], toff[a], toff[b]
        rc = chamfer_3D.nm_distance_ragged(q[q0:q1], qa, t[t0:t1], ta, dist[q0:q1], idx[q0:q1], search=search)
        if rc != 1:
            raise RuntimeError("chamfer_3D.nm_distance_ragged failed: " + _lib.last_error())
    return dist, idx


def chamfer_ragged(clouds1, clouds2, search=None):
    """Pair j: clouds1[j] [N_j,3] against clouds2[j] [M_j,3], float32 GPU tensors; each side a list, or packed as
    (points, offsets).  Returns (dist1, dist2, idx1, idx2, offsets1, offsets2): dist1 / idx1 packed like clouds1 -- the
    squared distance from each of its points to the nearest point of the pair's clouds2[j] and that point's index INSIDE
    clouds2[j] -- dist2 / idx2 the converse; offsets as int64 CPU tensors of c + 1 entries.  Per pair the bits of
    chamfer_3DDist on that pair alone, for finite clouds; a pair with an empty cloud on one side only is an error.
    Forward only.  search: None (the calling thread's ragged search, the grid search by default), "grid" or "dense" (all
    pairs, the same bits) for both directions of this call."""
    _lib.check_nn_ragged_search(search)
    p1, off1 = pack_clouds(clouds1, "clouds1")
    p2, off2 = pack_clouds(clouds2, "clouds2")
    if len(off1) != len(off2):
        raise ValueError("chamfer_ragged: %d clouds against %d" % (len(off1) - 1, len(off2) - 1))
    if p1.requires_grad or p2.requires_grad:
        raise RuntimeError("chamfer_ragged is forward only and an input requires grad: chamfer_raggedDist (ragged) and "
                           "chamfer_3DDist (rectangular) are the differentiable paths")
    _lib.require_gpu(p1, p2)
    if p1.device != p2.device:
        raise ValueError("chamfer_ragged: clouds1 and clouds2 are on different devices")
    dist1, idx1 = _one_way(p1, off1, p2, off2, search)
    dist2, idx2 = _one_way(p2, off2, p1, off1, search)
    return dist1, dist2, idx1, idx2, torch.tensor(off1, dtype=torch.int64), torch.tensor(off2, dtype=torch.int64)


class chamfer_raggedFunction(Function):
    """Packed points [T1,3], [T2,3] (float32, contiguous, one device) and their host offsets (c + 1 Python ints each, checked
    by the caller: chamfer_raggedDist does) -> dist1, dist2, idx1, idx2 as chamfer_ragged; differentiable in the points."""

    @staticmethod
    def forward(ctx, p1, p2, off1, off2):
        dist1, idx1 = _one_way(p1, off1, p2, off2)
        dist2, idx2 = _one_way(p2, off2, p1, off1)
        ctx.save_for_backward(p1, p2, idx1, idx2)
        ctx.offsets = (list(off1), list(off2))
        ctx.mark_non_differentiable(idx1, idx2)
        return dist1, dist2, idx1, idx2

    @staticmethod
    def backward(ctx, graddist1, graddist2, gradidx1, gradidx2):
        p1, p2, idx1, idx2 = ctx.saved_tensors
        off1, off2 = ctx.offsets
        graddist1 = graddist1.contiguous()
        graddist2 = graddist2.contiguous()
        gradxyz1 = torch.empty_like(p1)          # every row is overwritten: nothing to zero
        gradxyz2 = torch.empty_like(p2)
        for a, b, na, ma in chunks(chamfer_3D.RAGGED_MAX_PAIRS, off1, off2):
            n0, n1, m0, m1 = off1[a], off1[b], off2[a], off2[b]
            rc = chamfer_3D.backward_ragged(p1[n0:n1], na, p2[m0:m1], ma, gradxyz1[n0:n1], gradxyz2[m0:m1], graddist1[n0:n1],
                                            graddist2[m0:m1], idx1[n0:n1], idx2[m0:m1])
            if rc != 1:
                raise RuntimeError("chamfer_3D.backward_ragged failed: " + _lib.last_error())
        return gradxyz1, gradxyz2, None, None


class chamfer_raggedDist(nn.Module):
    """chamfer_ragged as a loss term: forward(clouds1, clouds2) takes what chamfer_ragged takes -- lists of [N_j,3] tensors
    or (points, offsets) -- returns what it returns, (dist1, dist2, idx1, idx2, offsets1, offsets2), and dist1 / dist2 carry
    the gradient to the points: to each element of a list (through torch.cat), or to the packed tensor."""

    def __init__(self):
        super(chamfer_raggedDist, self).__init__()

    def forward(self, clouds1, clouds2):
        p1, off1 = pack_clouds(clouds1, "clouds1")
        p2, off2 = pack_clouds(clouds2, "clouds2")
        if len(off1) != len(off2):
            raise ValueError("chamfer_raggedDist: %d clouds against %d" % (len(off1) - 1, len(off2) - 1))
        _lib.require_gpu(p1, p2)
        if p1.device != p2.device:
            raise ValueError("chamfer_raggedDist: clouds1 and clouds2 are on different devices")
        dist1, dist2, idx1, idx2 = chamfer_raggedFunction.apply(p1, p2, off1, off2)
        return dist1, dist2, idx1, idx2, torch.tensor(off1, dtype=torch.int64), torch.tensor(off2, dtype=torch.int64)
