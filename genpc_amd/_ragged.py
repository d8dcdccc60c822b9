"""What every ragged wrapper does before it calls the library: read a batch that comes as a list of clouds or packed as
(points, offsets), and cut S entries into library calls of at most `limit` with their offset tables counted from the call's
first entry."""
import ctypes

import torch

from . import chamfer_3D


def _is_offsets(x):
    if torch.is_tensor(x):
        return x.dim() == 1 and not x.dtype.is_floating_point and not x.dtype.is_complex
    if isinstance(x, (list, tuple)) or type(x).__name__ == "ndarray":
        return all(isinstance(v, int) or (hasattr(v, "dtype") and getattr(v, "ndim", 1) == 0 and "int" in str(v.dtype)) for v in x)
    return False


def is_packed(clouds):
    """Is this a packed batch, a tuple (points tensor, offsets), and not a list of clouds?"""
    return isinstance(clouds, tuple) and len(clouds) == 2 and torch.is_tensor(clouds[0]) and _is_offsets(clouds[1])


def pack_clouds(clouds, name="clouds"):
    """A ragged batch as (points [T,3] float32 contiguous, offsets: c + 1 Python ints).  ``clouds`` is a list of [N_j,3]
    tensors, or already packed: a tuple (points [T,3], offsets) with offsets a sequence of ints or a 1-D CPU int tensor."""
    if is_packed(clouds):
        points, off = clouds
        if torch.is_tensor(off):
            if off.is_cuda:
                raise ValueError("chamfer_ragged: the offsets of %s live on the host (a device tensor would have to be read back)" % name)
            off = off.tolist()
        off = [int(v) for v in off]
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError("chamfer_ragged: packed %s must be [T,3], got %s" % (name, tuple(points.shape)))
        if not off or off[0] != 0 or any(b < a for a, b in zip(off, off[1:])) or off[-1] != points.shape[0]:
            raise ValueError("chamfer_ragged: the offsets of %s must ascend from 0 to its %d points" % (name, points.shape[0]))
        if points.dtype != torch.float32:
            raise TypeError("chamfer_ragged: %s must be torch.float32, got %s" % (name, points.dtype))
        return points.contiguous(), off
    if not isinstance(clouds, (list, tuple)):
        raise TypeError("chamfer_ragged: %s is a list of [N,3] tensors or a tuple (points, offsets)" % name)
    off = [0]
    for j, t in enumerate(clouds):
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError("chamfer_ragged: %s[%d] must be an [N,3] tensor" % (name, j))
        if t.dtype != torch.float32:
            raise TypeError("chamfer_ragged: %s[%d] must be torch.float32, got %s" % (name, j, t.dtype))
        if t.device != clouds[0].device:
            raise ValueError("chamfer_ragged: %s[%d] is on %s, %s[0] on %s" % (name, j, t.device, name, clouds[0].device))
        off.append(off[-1] + t.shape[0])
    if len(clouds) == 0:
        return torch.empty((0, 3), dtype=torch.float32), off
    return torch.cat(list(clouds), dim=0).contiguous(), off


def ragged_side(clouds, fn, name="clouds"):
    """A ragged batch as (points [T,3] float32 contiguous, offsets: S + 1 Python ints): a list of [N_j,3] tensors or packed
    (points, offsets), as pack_clouds reads them; errors name `fn`."""
    if is_packed(clouds):
        points, off = clouds
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError("%s: packed %s must be [T,3], got %s" % (fn, name, tuple(points.shape)))
        if torch.is_tensor(off) and off.is_cuda:
            raise ValueError("%s: the offsets of %s live on the host (a device tensor would have to be read back)" % (fn, name))
        if points.dtype != torch.float32:
            raise TypeError("%s: packed %s must be torch.float32, got %s" % (fn, name, points.dtype))
        return pack_clouds(clouds, name)
    if not isinstance(clouds, (list, tuple)):
        raise TypeError("%s: %s is a list of [N,3] tensors or a tuple (points, offsets)" % (fn, name))
    for j, t in enumerate(clouds):
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError("%s: %s[%d] must be an [N,3] tensor" % (fn, name, j))
        if t.dtype != torch.float32:
            raise TypeError("%s: %s[%d] must be torch.float32, got %s" % (fn, name, j, t.dtype))
    return pack_clouds(clouds, name)


def host_ints(values, name="offsets"):
    """(a ctypes int array of the values, its void pointer -- which keeps the array alive); errors call the values `name`."""
    arr, _ = chamfer_3D._host_offsets(values, name)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def chunks(limit, *tables):
    """Cuts the S entries of parallel offset tables (S + 1 Python ints each) into library calls of at most `limit` entries:
    yields (a, b, table, ...) per call -- entries a .. b - 1, and each table's slice a .. b counted from its entry a."""
    s = len(tables[0]) - 1
    for a in range(0, s, limit):
        b = min(a + limit, s)
        yield (a, b) + tuple([v - off[a] for v in off[a:b + 1]] for off in tables)
