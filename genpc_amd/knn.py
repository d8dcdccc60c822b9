"""Exact k-nearest-neighbour query on the HIP library (csrc/knn_query.hip) -- what the reference asks of
scipy's ``KDTree.query`` in ``linear_interpolation`` (utils/dataUtils.py:128-134).  GPU only: there is no fallback."""
import torch

from . import _lib

_L = _lib.lib
_p = _lib.ptr
MAX_K = 32


def knn_query(queries, targets, k):
    """The k nearest targets of every query: ``(dist2, idx)`` with a trailing k axis, float32 squared distances and
    int32 indices into ``targets``.  queries [N,3] with targets [M,3], or [B,N,3] with [B,M,3]; float32 GPU tensors.

    Distances ascend; among bit-equal distances the lower index comes first, and the same order decides which of several
    equal candidates holds the k-th place.  Column 0 holds the bits of ``chamfer_3D.nm_distance``.  Only targets at a
    distance < +inf are listed: slots past them (fewer than k targets, non-finite input) hold ``(+inf, -1)``."""
    k = int(k)
    if k < 1 or k > MAX_K:
        raise ValueError("knn_query: k must be 1 .. %d, got %d" % (MAX_K, k))
    _lib.require_gpu(queries, targets)
    if queries.dim() != targets.dim() or queries.dim() not in (2, 3) or queries.shape[-1] != 3 or targets.shape[-1] != 3:
        raise ValueError("knn_query: queries [N,3] with targets [M,3], or [B,N,3] with [B,M,3]")
    single = queries.dim() == 2
    q = queries.unsqueeze(0) if single else queries
    t = targets.unsqueeze(0) if single else targets
    if q.shape[0] != t.shape[0]:
        raise ValueError("knn_query: batch sizes differ (%d, %d)" % (q.shape[0], t.shape[0]))
    if q.device != t.device:
        raise ValueError("knn_query: queries and targets are on different devices")
    q, t = q.contiguous(), t.contiguous()
    _lib.check_tensors((("queries", q), ("targets", t)))
    b, nq, _ = q.shape
    nt = t.shape[1]
    if nt < 1 and b * nq > 0:
        raise ValueError("knn_query: no targets")
    dist = torch.empty((b, nq, k), dtype=torch.float32, device=q.device)
    idx = torch.empty((b, nq, k), dtype=torch.int32, device=q.device)
    rc = _lib.on_device_of(q, _L.genpc_knn_query, b, nq, _p(q), nt, _p(t), k, _p(dist), _p(idx))
    if rc != 1:
        raise RuntimeError("genpc_knn_query failed (%d): %s" % (rc, _lib.last_error()))
    return (dist[0], idx[0]) if single else (dist, idx)
