"""The host side of the ragged auction EMD, without a GPU: genpc_emd_forward_ragged / genpc_emd_backward_ragged are declared,
bound and exported and the ABI version stands; every refusal of the C entry points comes back as -1 with its message before
anything touches a device (null stream, dummy pointers: nothing is enqueued); and what the Python packers refuse."""
import ctypes

import pytest
import torch

from test_abi import header_prototypes

DUMMY = ctypes.c_void_p(0x1000)          # never dereferenced: every case below is decided on the host
NULL = ctypes.c_void_p(0)


@pytest.fixture(scope="module")
def L():
    from genpc_amd import build
    build.build(verbose=False)
    from genpc_amd import _lib
    return _lib


def offs(*v):
    return (ctypes.c_int * len(v))(*v)


def fwd(L, c, off, ptr=DUMMY, iters=5, **null):
    names = ("xyz1", "xyz2", "dist", "assignment", "price", "assignment_inv", "bid", "bid_increments", "max_increments", "max_idx")
    args = [NULL if null.get(k) else ptr for k in names]
    return L.lib.genpc_emd_forward_ragged(c, off, *args, 0.005, iters, None)


def bwd(L, c, off, ptr=DUMMY, **null):
    names = ("xyz1", "xyz2", "gradxyz", "graddist", "idx")
    args = [NULL if null.get(k) else ptr for k in names]
    return L.lib.genpc_emd_backward_ragged(c, off, *args, None)


def test_declared_bound_and_exported(L):
    p = header_prototypes()
    assert p.get("genpc_emd_forward_ragged") == 15          # c, off, 2 clouds, 8 state arrays, eps, iters + stream
    assert p.get("genpc_emd_backward_ragged") == 8
    assert len(L.SIGNATURES["genpc_emd_forward_ragged"][1]) == 15
    assert len(L.SIGNATURES["genpc_emd_backward_ragged"][1]) == 8
    assert set(p) == set(L.SIGNATURES)
    assert L.lib.genpc_emd_forward_ragged is not None and L.lib.genpc_emd_backward_ragged is not None
    assert L.ABI_VERSION == 28 and L.lib.genpc_abi_version() == 28      # additive: the number stayed 27 (28: genpc_hpr_plan)


CASES = [
    ("negative number of pairs", -1, offs(0)),
    ("more than 384 pairs", 385, offs(*([0] * 386))),
    ("null offset table", 2, None),
    ("offsets must start at 0", 2, offs(256, 512, 768)),
    ("offsets must ascend", 2, offs(0, 512, 256)),
    ("pair 1 has 100 points, not a multiple of 256", 3, offs(0, 256, 356, 612)),
    ("pair 0 has 255 points, not a multiple of 256", 1, offs(0, 255)),
    ("more than 2^28 points", 2, offs(0, 1 << 28, (1 << 28) + 256)),
]


@pytest.mark.parametrize("msg,c,off", CASES, ids=[c[0] for c in CASES])
def test_refusals_forward_and_backward(L, msg, c, off):
    assert fwd(L, c, off) == -1
    err = L.last_error()
    assert err.startswith("genpc_emd_forward_ragged: ") and msg in err, err
    assert bwd(L, c, off) == -1
    err = L.last_error()
    assert err.startswith("genpc_emd_backward_ragged: ") and msg in err, err


def test_negative_rounds_are_refused(L):
    assert fwd(L, 1, offs(0, 256), iters=-1) == -1
    assert "negative number of rounds" in L.last_error()
    assert fwd(L, 0, None, iters=-1) == -1


@pytest.mark.parametrize("name", ["xyz1", "xyz2", "dist", "assignment", "price", "assignment_inv", "bid", "bid_increments",
                                  "max_increments", "max_idx"])
def test_a_null_device_pointer_with_work_to_do_is_refused(L, name):
    assert fwd(L, 2, offs(0, 256, 256), **{name: True}) == -1
    assert L.last_error() == "genpc_emd_forward_ragged: null pointer"


@pytest.mark.parametrize("name", ["xyz1", "xyz2", "gradxyz", "graddist", "idx"])
def test_backward_null_pointer(L, name):
    assert bwd(L, 1, offs(0, 512), **{name: True}) == -1
    assert L.last_error() == "genpc_emd_backward_ragged: null pointer"


def test_nothing_to_do_returns_1(L):
    assert fwd(L, 0, None, ptr=NULL) == 1                    # no pair: not even the table is looked at
    assert bwd(L, 0, None, ptr=NULL) == 1
    assert fwd(L, 3, offs(0, 0, 0, 0), ptr=NULL) == 1        # pairs without points are legal and write nothing
    assert bwd(L, 3, offs(0, 0, 0, 0), ptr=NULL) == 1
    assert fwd(L, 384, offs(*([0] * 385)), ptr=NULL, iters=0) == 1


def clouds(*sizes):
    return [torch.arange(n * 3, dtype=torch.float32).reshape(n, 3) for n in sizes]


def test_python_packers_refuse_cpu_tensors_and_bad_pairs(L):
    from genpc_amd import emd, metric
    from genpc_amd.loss_functions import emd_raggedDist
    from genpc_amd.loss_functions.emd.emd_ragged import emd_raggedFunction      # noqa: F401  (the name exists)
    from genpc_amd.utils.loss_util import emd_ragged_loss
    m = emd_raggedDist()
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        m(clouds(256, 512), clouds(256, 512), 0.005, 2)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        m((torch.zeros(768, 3), [0, 256, 768]), (torch.zeros(768, 3), [0, 256, 768]), 0.005, 2)
    with pytest.raises(ValueError, match=r"pair 1 has 512 points against 256"):
        m(clouds(256, 512), clouds(256, 256), 0.005, 2)
    with pytest.raises(ValueError, match=r"pair 2 has 100 points, not a multiple of 256"):
        m(clouds(256, 0, 100), clouds(256, 0, 100), 0.005, 2)
    with pytest.raises(ValueError, match="3 clouds against 2"):
        m(clouds(256, 256, 256), clouds(256, 256), 0.005, 2)
    with pytest.raises(ValueError, match=r"clouds2\[0\] must be an \[N,3\] tensor"):
        m(clouds(256), [torch.zeros(256, 2)], 0.005, 2)
    with pytest.raises(TypeError):
        m([c.double() for c in clouds(256)], clouds(256), 0.005, 2)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        emd_ragged_loss(clouds(256), clouds(256))
    with pytest.raises(ValueError, match=r"evaluate_scans_ragged: pair 0 has 256 points against 512"):
        metric.evaluate_scans_ragged(clouds(256), clouds(512))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        metric.evaluate_scans_ragged(clouds(256), clouds(256))
    z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        emd.forward_ragged(torch.zeros(256, 3), torch.zeros(256, 3), [0, 256], z(256), z(256, torch.int32), z(256), z(256, torch.int32),
                           z(256, torch.int32), z(256), z(256), z(256, torch.int32), 0.005, 2)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        emd.backward_ragged(torch.zeros(256, 3), torch.zeros(256, 3), [0, 256], torch.zeros(256, 3), z(256), z(256, torch.int32))
