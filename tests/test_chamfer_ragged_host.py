"""The host side of the differentiable ragged Chamfer, without a GPU: what chamfer_3D.backward_ragged, chamfer_raggedDist and
chamfer_ragged_loss refuse before any library call, and that chamfer_ragged itself is still forward only."""
import pytest
import torch


@pytest.fixture(scope="module")
def ragged():
    from genpc_amd.loss_functions.Chamfer3D import dist_chamfer_ragged
    return dist_chamfer_ragged


def clouds(*sizes):
    return [torch.zeros(n, 3) for n in sizes]


def test_the_library_has_the_entry_point():
    from genpc_amd import _lib
    assert _lib.ABI_VERSION >= 22 and _lib.lib.genpc_abi_version() == _lib.ABI_VERSION
    assert "genpc_chamfer_backward_ragged" in _lib.SIGNATURES and len(_lib.SIGNATURES["genpc_chamfer_backward_ragged"][1]) == 12


def test_refusals_of_the_library_need_no_gpu():
    """The offsets are checked before anything is enqueued: -1 and the function's name, with no device in the machine."""
    import ctypes
    from genpc_amd import _lib
    vp = lambda xs: ctypes.cast((ctypes.c_int * len(xs))(*xs), ctypes.c_void_p)      # noqa: E731
    null = ctypes.c_void_p(0)
    for c, noff, moff in ((2, [0, 10, 20], [0, 30, 30]), (2, [0, 20, 20], [0, 10, 30]), (2, [0, 15, 10], [0, 10, 30]),
                          (2, [5, 10, 20], [0, 10, 30]), (-1, [0], [0]), (385, [0] * 386, [0] * 386)):
        a, b = vp(noff), vp(moff)
        assert _lib.lib.genpc_chamfer_backward_ragged(c, a, null, b, null, null, null, null, null, null, null, null) == -1
        assert "genpc_chamfer_backward_ragged" in _lib.last_error()
    assert _lib.lib.genpc_chamfer_backward_ragged(0, null, null, null, null, null, null, null, null, null, null, null) == 1
    a, b = vp([0, 0, 0]), vp([0, 0, 0])
    assert _lib.lib.genpc_chamfer_backward_ragged(2, a, null, b, null, null, null, null, null, null, null, null) == 1
    a, b = vp([0, 4]), vp([0, 4])
    assert _lib.lib.genpc_chamfer_backward_ragged(1, a, null, b, null, null, null, null, null, null, null, null) == -1      # null pointers with work to do
    assert "null pointer" in _lib.last_error()


def test_backward_ragged_refuses_cpu_tensors_dtypes_counts_and_device_offsets():
    from genpc_amd import chamfer_3D
    f = lambda *s: torch.zeros(*s)                                                   # noqa: E731
    i = lambda n: torch.zeros(n, dtype=torch.int32)                                   # noqa: E731
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        chamfer_3D.backward_ragged(f(8, 3), [0, 3, 8], f(6, 3), [0, 4, 6], f(8, 3), f(6, 3), f(8), f(6), i(8), i(6))
    meta = lambda *s, **k: torch.zeros(*s, device="meta", **k)                        # noqa: E731
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        chamfer_3D.backward_ragged(meta(8, 3), [0, 3, 8], f(6, 3), [0, 4, 6], f(8, 3), f(6, 3), f(8), f(6), i(8), i(6))


def test_module_refuses_what_chamfer_ragged_refuses(ragged):
    m = ragged.chamfer_raggedDist()
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        m(clouds(3, 5), clouds(4, 2))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        m((torch.zeros(8, 3, requires_grad=True), [0, 3, 8]), (torch.zeros(6, 3), [0, 4, 6]))
    with pytest.raises(ValueError, match="3 clouds against 2"):
        m(clouds(3, 5, 1), clouds(4, 2))
    with pytest.raises(ValueError, match="2 clouds against 1"):
        m((torch.zeros(8, 3), [0, 3, 8]), clouds(4))
    with pytest.raises(TypeError, match="float32"):
        m(clouds(3), [torch.zeros(4, 3, dtype=torch.float64)])
    with pytest.raises(ValueError, match=r"must be an \[N,3\] tensor"):
        m([torch.zeros(3, 3), torch.zeros(5, 2)], clouds(4, 2))
    with pytest.raises(ValueError, match="must ascend from 0 to its 8 points"):
        m((torch.zeros(8, 3), [0, 5, 3]), clouds(4, 2))
    with pytest.raises(TypeError):
        m(torch.zeros(2, 8, 3), clouds(4, 2))


class _DeviceOffsets:
    """What _host_offsets asks of a tensor, answering as a GPU tensor would (there is no GPU in this process)."""
    is_cuda = True
    device = "cuda:0"


def test_device_offsets_are_refused():
    """Offsets live on the host: a device tensor would have to be read back."""
    from genpc_amd import chamfer_3D
    with pytest.raises(ValueError, match="noff lives on the host"):
        chamfer_3D._host_offsets(_DeviceOffsets(), "noff")
    with pytest.raises(TypeError, match="1-D integer tensor"):
        chamfer_3D._host_offsets(torch.zeros(3), "noff")
    with pytest.raises(ValueError, match="needs c \\+ 1 entries"):
        chamfer_3D._host_offsets([], "noff")


def test_loss_refuses_unknown_kinds_and_cpu_tensors():
    from genpc_amd.utils.loss_util import chamfer_ragged_loss
    with pytest.raises(ValueError, match="'l1' or 'l2'"):
        chamfer_ragged_loss(clouds(3), clouds(4), kind="emd")
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        chamfer_ragged_loss(clouds(3, 5), clouds(4, 2))
    with pytest.raises(ValueError, match="3 clouds against 2"):
        chamfer_ragged_loss(clouds(3, 5, 1), clouds(4, 2), kind="l2")


def test_chamfer_ragged_is_still_forward_only(ragged):
    a = clouds(3, 5)
    a[1].requires_grad_(True)
    with pytest.raises(RuntimeError, match="chamfer_3DDist"):
        ragged.chamfer_ragged(a, clouds(4, 2))
    with pytest.raises(RuntimeError, match="chamfer_raggedDist"):
        ragged.chamfer_ragged(clouds(4, 2), (torch.zeros(8, 3, requires_grad=True), [0, 3, 8]))
