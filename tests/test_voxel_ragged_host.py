"""The host side of the ragged voxel grid, without a GPU: genpc_voxel_down_sample_ragged is declared, bound and exported and
the ABI version stands; every refusal of the C entry point comes back as -1 with its message before anything touches a device
(null stream, dummy pointers: nothing is enqueued); and what reg_xyz.voxel_down_sample_clouds refuses."""
import ctypes

import pytest
import torch

from test_abi import header_prototypes

DUMMY = ctypes.c_void_p(0x1000)          # never dereferenced: every case below is decided on the host
NULL = ctypes.c_void_p(0)
PREFIX = "genpc_voxel_down_sample_ragged: "


@pytest.fixture(scope="module")
def L():
    from genpc_amd import build
    build.build(verbose=False)
    from genpc_amd import _lib
    return _lib


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def doubles(*v):
    return (ctypes.c_double * len(v))(*v)


def call(L, c, off, sizes, ptr=DUMMY):
    cast = lambda a: NULL if a is None else ctypes.cast(a, ctypes.c_void_p)
    return L.lib.genpc_voxel_down_sample_ragged(c, cast(off), ptr, ptr, cast(sizes), ptr, ptr, ptr, None)


def max_clouds():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = re.search(r"#define\s+GENPC_VOXEL_RAGGED_MAX_CLOUDS\s+(\d+)", open(os.path.join(root, "include", "genpc_hip.h")).read())
    assert m, "the header exports the bound as a constant"
    return int(m.group(1))


def test_declared_bound_and_exported(L):
    p = header_prototypes()
    assert p.get("genpc_voxel_down_sample_ragged") == 9          # c, off, xyz, colors, voxel_sizes, out, out_colors, out_counts + stream
    assert len(L.SIGNATURES["genpc_voxel_down_sample_ragged"][1]) == 9
    assert set(p) == set(L.SIGNATURES)
    assert L.lib.genpc_voxel_down_sample_ragged is not None
    assert L.ABI_VERSION == 28 and L.lib.genpc_abi_version() == 28      # additive: the number stays
    from genpc_amd import reg_xyz
    assert max_clouds() >= 256 and reg_xyz.VOXEL_RAGGED_MAX_CLOUDS == max_clouds()


def test_refusals(L):
    n = max_clouds()
    cases = [
        ("negative number of clouds", -1, ints(0), doubles(0.03)),
        ("more than %d clouds" % n, n + 1, ints(*([0] * (n + 2))), doubles(*([0.03] * (n + 1)))),
        ("null offset or voxel size table", 2, None, doubles(0.03, 0.03)),
        ("null offset or voxel size table", 2, ints(0, 5, 9), None),
        ("offsets must start at 0", 2, ints(1, 5, 9), doubles(0.03, 0.03)),
        ("offsets must ascend", 2, ints(0, 9, 5), doubles(0.03, 0.03)),
        ("more than 2^28 points", 2, ints(0, 1 << 28, (1 << 28) + 1), doubles(0.03, 0.03)),
        ("the voxel size of cloud 1 is not > 0", 3, ints(0, 5, 9, 12), doubles(0.03, 0.0, 0.02)),
        ("the voxel size of cloud 2 is not > 0", 3, ints(0, 5, 9, 12), doubles(0.03, 0.02, -1.0)),
        ("the voxel size of cloud 0 is not > 0", 1, ints(0, 5), doubles(float("nan"))),
    ]
    for msg, c, off, sizes in cases:
        assert call(L, c, off, sizes) == -1, msg
        err = L.last_error()
        assert err.startswith(PREFIX) and msg in err, (msg, err)


def test_a_null_device_pointer_with_work_to_do_is_refused(L):
    assert call(L, 1, ints(0, 5), doubles(0.03), ptr=NULL) == -1
    assert L.last_error() == PREFIX + "null pointer"


def test_no_cloud_returns_1(L):
    assert call(L, 0, None, None, ptr=NULL) == 1             # not even the tables are looked at


def test_the_limit_itself_is_not_refused_for_its_number(L):
    n = max_clouds()
    assert call(L, n, ints(*([0] * n + [1])), doubles(*([0.03] * (n - 1) + [0.0]))) == -1
    assert "the voxel size of cloud %d is not > 0" % (n - 1) in L.last_error()


def clouds(*sizes):
    return [torch.arange(n * 3, dtype=torch.float32).reshape(n, 3) for n in sizes]


def test_the_python_wrapper_refuses(L):
    from genpc_amd import reg_xyz
    f = reg_xyz.voxel_down_sample_clouds
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        f(clouds(5, 7), 0.03)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        f((torch.zeros(12, 3), [0, 5, 12]), [0.03, 0.02])
    with pytest.raises(TypeError, match="float32"):
        f([c.double() for c in clouds(5)], 0.03)
    with pytest.raises(ValueError, match=r"clouds\[1\] must be an \[N,3\] tensor"):
        f([torch.zeros(5, 3), torch.zeros(5, 2)], 0.03)
    with pytest.raises(ValueError, match=r"packed clouds must be \[T,3\]"):
        f((torch.zeros(12, 2), [0, 5, 12]), 0.03)
    with pytest.raises(ValueError, match="2 voxel sizes for 3 clouds"):
        f(clouds(5, 7, 9), [0.03, 0.02])
    with pytest.raises(ValueError, match="the voxel size of cloud 1 must be positive"):
        f(clouds(5, 7), [0.03, 0.0])
    with pytest.raises(ValueError, match="colors must be"):
        f(clouds(5, 7), 0.03, colors=clouds(5, 6))
    with pytest.raises(ValueError, match="colors must be"):
        f(clouds(5, 7), 0.03, colors=clouds(5))
    assert f([], 0.03) == [] and f([], 0.03, colors=[]) == ([], [])
    if torch.cuda.is_available():          # (a device tensor cannot be made without a device)
        with pytest.raises(ValueError, match="offsets of clouds live on the host"):
            f((torch.zeros(12, 3, device="cuda"), torch.tensor([0, 5, 12], device="cuda")), 0.03)
