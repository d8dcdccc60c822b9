"""Drop-in for the reference's pybind module ``chamfer_3D``
(loss_functions/Chamfer3D/chamfer_cuda.cpp:30-33): same two functions, same
argument order, same caller-allocates contract, same return codes -- but the
work is done by libgenpc_hip.so through its C ABI, on torch's current stream.
Unlike the reference (dist_chamfer_3D.py:45 ignores the code) callers in this
package raise on a non-1 return.
"""
import ctypes

from . import _lib

_L = _lib.lib
_p = _lib.ptr
RAGGED_MAX_PAIRS = 384          # include/genpc_hip.h: pairs per genpc_nm_distance_ragged / genpc_chamfer_backward_ragged call


def forward(xyz1, xyz2, dist1, dist2, idx1, idx2):
    """chamfer_cuda.cpp:17-19 -> chamfer3D.cu:136-154."""
    _lib.check_tensors((("xyz1", xyz1), ("xyz2", xyz2), ("dist1", dist1), ("dist2", dist2)),
                       (("idx1", idx1), ("idx2", idx2)))
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    return _lib.on_device_of(xyz1, _L.genpc_chamfer_forward, b, n, _p(xyz1), m, _p(xyz2), _p(dist1), _p(idx1),
                             _p(dist2), _p(idx2))


def backward(xyz1, xyz2, gradxyz1, gradxyz2, graddist1, graddist2, idx1, idx2):
    """chamfer_cuda.cpp:22-26 -> chamfer3D.cu:176-195."""
    _lib.check_tensors((("xyz1", xyz1), ("xyz2", xyz2), ("gradxyz1", gradxyz1), ("gradxyz2", gradxyz2),
                        ("graddist1", graddist1), ("graddist2", graddist2)), (("idx1", idx1), ("idx2", idx2)))
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    return _lib.on_device_of(xyz1, _L.genpc_chamfer_backward, b, n, _p(xyz1), m, _p(xyz2), _p(graddist1), _p(idx1),
                             _p(graddist2), _p(idx2), _p(gradxyz1), _p(gradxyz2))


def nm_distance(xyz, xyz2, result, result_i):
    """One direction only (NmDistanceKernel, chamfer3D.cu:12-134)."""
    _lib.check_tensors((("xyz", xyz), ("xyz2", xyz2), ("result", result)), (("result_i", result_i),))
    b, n, _ = xyz.shape
    m = xyz2.shape[1]
    return _lib.on_device_of(xyz, _L.genpc_nm_distance, b, n, _p(xyz), m, _p(xyz2), _p(result), _p(result_i))


def nm_distance_within(xyz, xyz2, radius2, result, result_i):
    """nm_distance with a search limit (squared): queries without a target within it get
    (+inf, -1); the others exactly what nm_distance returns (reg_xyz.py:41-52)."""
    _lib.check_tensors((("xyz", xyz), ("xyz2", xyz2), ("result", result)), (("result_i", result_i),))
    b, n, _ = xyz.shape
    m = xyz2.shape[1]
    return _lib.on_device_of(xyz, _L.genpc_nm_distance_within, b, n, _p(xyz), m, _p(xyz2), float(radius2), _p(result),
                             _p(result_i))


def _host_offsets(off, name):
    """Offsets as a ctypes int array: a Python int sequence or a CPU integer tensor (a device tensor would have to be read back)."""
    if hasattr(off, "is_cuda"):
        if off.is_cuda:
            raise ValueError("genpc_amd: %s lives on the host (a CPU int tensor or a sequence of ints), got a %s tensor" % (name, off.device))
        if off.dim() != 1 or off.dtype.is_floating_point:
            raise TypeError("genpc_amd: %s must be a 1-D integer tensor" % name)
        off = off.tolist()
    off = [int(v) for v in off]
    if not off:
        raise ValueError("genpc_amd: %s needs c + 1 entries, got none" % name)
    if any(v < -2 ** 31 or v >= 2 ** 31 for v in off):
        raise ValueError("genpc_amd: %s does not fit 32-bit ints" % name)
    return (ctypes.c_int * len(off))(*off), off


def nm_distance_ragged(xyz, noff, xyz2, moff, result, result_i, search=None):
    """nm_distance over a ragged batch (genpc_nm_distance_ragged): pair j has the queries xyz[noff[j]:noff[j+1]] and the
    targets xyz2[moff[j]:moff[j+1]]; xyz [N,3], xyz2 [M,3], result [N], result_i [N] packed in pair order, result_i
    counted inside the pair's own targets.  noff, moff: c + 1 ints each, Python sequences or CPU int tensors.
    search: None leaves the calling thread's ragged search alone (the grid search unless genpc_nn_ragged_tune was called);
    "grid" or "dense" (all pairs, csrc/nn_ragged_dense.hip: the same bits) holds for this call and is restored behind it."""
    _lib.check_nn_ragged_search(search)
    _lib.check_tensors((("xyz", xyz), ("xyz2", xyz2), ("result", result)), (("result_i", result_i),))
    na, nl = _host_offsets(noff, "noff")
    ma, ml = _host_offsets(moff, "moff")
    if len(nl) != len(ml):
        raise ValueError("genpc_amd: noff and moff differ in length (%d, %d)" % (len(nl), len(ml)))
    # the library checks the offsets against each other; only the caller's buffers can be checked against them, here
    for name, t, rows in (("xyz", xyz, nl[-1]), ("xyz2", xyz2, ml[-1])):
        if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] != rows:
            raise ValueError("genpc_amd: %s must be [%d,3] (the last offset), got %s" % (name, rows, tuple(t.shape)))
    if result.numel() != nl[-1] or result_i.numel() != nl[-1]:
        raise ValueError("genpc_amd: result and result_i must hold noff[-1] = %d elements" % nl[-1])
    with _lib.nn_ragged_search(search):
        return _lib.on_device_of(xyz, _L.genpc_nm_distance_ragged, len(nl) - 1, ctypes.cast(na, ctypes.c_void_p), _p(xyz),
                                 ctypes.cast(ma, ctypes.c_void_p), _p(xyz2), _p(result), _p(result_i))


def backward_ragged(xyz1, noff, xyz2, moff, gradxyz1, gradxyz2, graddist1, graddist2, idx1, idx2):
    """Both Chamfer gradients over a ragged batch (genpc_chamfer_backward_ragged): clouds and offsets as for
    nm_distance_ragged, graddist1 / idx1 [N] and graddist2 / idx2 [M] packed like their clouds with the indices counted inside
    the pair's own other cloud, as the ragged forward returns them.  gradxyz1 [N,3] and gradxyz2 [M,3] are OVERWRITTEN (no
    need to zero them), every row summed in a fixed order: the same bits on every run."""
    _lib.check_tensors((("xyz1", xyz1), ("xyz2", xyz2), ("gradxyz1", gradxyz1), ("gradxyz2", gradxyz2),
                        ("graddist1", graddist1), ("graddist2", graddist2)), (("idx1", idx1), ("idx2", idx2)))
    na, nl = _host_offsets(noff, "noff")
    ma, ml = _host_offsets(moff, "moff")
    if len(nl) != len(ml):
        raise ValueError("genpc_amd: noff and moff differ in length (%d, %d)" % (len(nl), len(ml)))
    # the library checks the offsets against each other; only the caller's buffers can be checked against them, here
    for name, t, rows in (("xyz1", xyz1, nl[-1]), ("xyz2", xyz2, ml[-1]), ("gradxyz1", gradxyz1, nl[-1]), ("gradxyz2", gradxyz2, ml[-1])):
        if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] != rows:
            raise ValueError("genpc_amd: %s must be [%d,3] (the last offset), got %s" % (name, rows, tuple(t.shape)))
    for name, t, rows in (("graddist1", graddist1, nl[-1]), ("idx1", idx1, nl[-1]), ("graddist2", graddist2, ml[-1]), ("idx2", idx2, ml[-1])):
        if t.numel() != rows:
            raise ValueError("genpc_amd: %s must hold %d elements (the last offset), got %d" % (name, rows, t.numel()))
    return _lib.on_device_of(xyz1, _L.genpc_chamfer_backward_ragged, len(nl) - 1, ctypes.cast(na, ctypes.c_void_p), _p(xyz1),
                             ctypes.cast(ma, ctypes.c_void_p), _p(xyz2), _p(graddist1), _p(idx1), _p(graddist2), _p(idx2),
                             _p(gradxyz1), _p(gradxyz2))
