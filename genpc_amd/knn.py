"""Exact k-nearest-neighbour query on the HIP library (csrc/knn_query.hip) -- what the reference asks of
scipy's ``KDTree.query`` in ``linear_interpolation`` (utils/dataUtils.py:128-134).  GPU only: there is no fallback."""
import torch

from . import _lib

_L = _lib.lib
_p = _lib.ptr
MAX_K = 32
RAGGED_MAX_PAIRS = 384          # include/genpc_hip.h: pairs per genpc_knn_query_ragged call


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


def knn_query_ragged(queries, targets, k):
    """``knn_query`` for S (queries, targets) pairs of any sizes.  Each side is a list of [N_j,3] float32 GPU tensors, or
    packed as (points [T,3], offsets) with S + 1 host ints (read as ``reg_xyz.knn_mean_distance_ragged`` reads its clouds).
    Returns a list of S pairs ``(dist2 [N_j,k], idx [N_j,k])``, views of one packed result -- float32 squared distances and
    int32 indices INSIDE pair j's own targets; pair j's are the bits of ``knn_query(queries[j], targets[j], k)``.  When the
    QUERIES came packed the return value is ``(pairs, (dist2 [T,k], idx [T,k]))``: the same list and the packed result
    it views, rows in the order of the packed queries.

    One library call per 384 pairs (genpc_knn_query_ragged: three launches each), nothing waits for the result.  A pair
    without queries gives empty tensors and may have no targets; a pair with queries and no targets is an error.  ``[]``
    against ``[]`` gives ``[]``."""
    from ._ragged import chunks, host_ints, is_packed, ragged_side
    k = int(k)
    if k < 1 or k > MAX_K:
        raise ValueError("knn_query_ragged: k must be 1 .. %d, got %d" % (MAX_K, k))
    packed = is_packed(queries)
    q, qoff = ragged_side(queries, "knn_query_ragged", "queries")
    t, toff = ragged_side(targets, "knn_query_ragged", "targets")
    if len(qoff) != len(toff):
        raise ValueError("knn_query_ragged: %d queries against %d targets" % (len(qoff) - 1, len(toff) - 1))
    s = len(qoff) - 1
    for j in range(s):
        if qoff[j + 1] > qoff[j] and toff[j + 1] == toff[j]:
            raise ValueError("knn_query_ragged: pair %d has %d queries and no targets" % (j, qoff[j + 1] - qoff[j]))
    if s == 0:                                 # (no pair: nothing to ask the library)
        return ([], (q.new_empty((0, k)), q.new_empty((0, k), dtype=torch.int32))) if packed else []
    _lib.require_gpu(q, t)
    if q.device != t.device:
        raise ValueError("knn_query_ragged: queries and targets are on different devices")
    dist = torch.empty((q.shape[0], k), dtype=torch.float32, device=q.device)
    idx = torch.empty((q.shape[0], k), dtype=torch.int32, device=q.device)
    for a, b, na, ma in chunks(RAGGED_MAX_PAIRS, qoff, toff):
        rc = _lib.on_device_of(q, _L.genpc_knn_query_ragged, b - a, host_ints(na)[1], _p(q[qoff[a]:qoff[b]]), host_ints(ma)[1],
                               _p(t[toff[a]:toff[b]]), k, _p(dist[qoff[a]:qoff[b]]), _p(idx[qoff[a]:qoff[b]]))
        if rc != 1:
            raise RuntimeError("genpc_knn_query_ragged failed (%d): %s" % (rc, _lib.last_error()))
    pairs = [(dist[qoff[j]:qoff[j + 1]], idx[qoff[j]:qoff[j + 1]]) for j in range(s)]
    return (pairs, (dist, idx)) if packed else pairs
