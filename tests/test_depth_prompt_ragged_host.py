"""The host side of the batched stage 1, without a GPU: the three entry points are declared, bound and exported; their refusals
come back as -1 with the function's name before anything touches a device; the exported plan is the header's; and what
DepthPrompting.getDepths, ScaleAdapter.colorPoints and pipeline.complete_scans_batched refuse, each naming itself."""
import ctypes
from types import SimpleNamespace

import numpy as np
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


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def cast(a):
    return NULL if a is None else ctypes.cast(a, ctypes.c_void_p)


def call(L, c, off, res=64, ps=1, rate=3, ptr=DUMMY):
    return L.lib.genpc_depth_prompt_ragged(c, cast(off), ptr, ptr, ptr, ptr, 1.0, 1e-2, 1e2, 1, 0.7, res, ps, rate,
                                           ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, None)


def test_declared_bound_and_exported(L):
    p = header_prototypes()
    assert p.get("genpc_depth_prompt_ragged") == 23
    assert p.get("genpc_depth_prompt_ragged_plan") == 6
    assert p.get("genpc_gather_colors_ragged") == 12
    for name in ("genpc_depth_prompt_ragged", "genpc_depth_prompt_ragged_plan", "genpc_gather_colors_ragged"):
        assert len(L.SIGNATURES[name][1]) == p[name] and getattr(L.lib, name) is not None
    assert set(p) == set(L.SIGNATURES)
    assert L.lib.genpc_abi_version() == L.ABI_VERSION


def test_refusals(L):
    ok = ints(0, 5, 9)
    cases = [("negative number of scans", dict(c=-1, off=ok)), ("more than 256 scans", dict(c=257, off=ints(*([0] * 258)))),
             ("null offset table", dict(c=2, off=None)), ("offsets must start at 0", dict(c=2, off=ints(1, 5, 9))),
             ("offsets must ascend", dict(c=2, off=ints(0, 9, 5))), ("more than 2^28 points", dict(c=2, off=ints(0, 1 << 28, (1 << 28) + 1))),
             ("res outside", dict(c=2, off=ok, res=0)), ("res outside", dict(c=2, off=ok, res=4097)),
             ("must be positive", dict(c=2, off=ok, ps=0)), ("must be positive", dict(c=2, off=ok, rate=0)),
             ("above 32", dict(c=2, off=ok, ps=11, rate=3)), ("owner planes", dict(c=256, off=ints(*([0] * 257)), res=4096)),
             ("null pointer", dict(c=2, off=ok, ptr=NULL))]
    for msg, kw in cases:
        assert call(L, **kw) == -1, msg
        err = L.last_error()
        assert err.startswith("genpc_depth_prompt_ragged: ") and msg in err, (msg, err)
    assert call(L, 0, None, ptr=NULL) == 1                     # no scan: nothing is looked at


def test_gather_refusals(L):
    f = L.lib.genpc_gather_colors_ragged
    ok = ints(0, 5, 9)
    for msg, args in (("negative number of scans", (-1, cast(ok), DUMMY, DUMMY, 3, 64, 64, 64.0, 63, NULL, DUMMY)),
                      ("more than 256 scans", (257, cast(ints(*([0] * 258))), DUMMY, DUMMY, 3, 64, 64, 64.0, 63, NULL, DUMMY)),
                      ("null offset table", (2, NULL, DUMMY, DUMMY, 3, 64, 64, 64.0, 63, NULL, DUMMY)),
                      ("offsets must ascend", (2, cast(ints(0, 9, 5)), DUMMY, DUMMY, 3, 64, 64, 64.0, 63, NULL, DUMMY)),
                      ("pixel grid exceeds", (2, cast(ok), DUMMY, DUMMY, 3, 64, 64, 65.0, 64, NULL, DUMMY)),
                      ("pixel grid exceeds", (2, cast(ok), DUMMY, DUMMY, 3, 64, 32, 64.0, 63, NULL, DUMMY)),
                      ("null pointer", (2, cast(ok), NULL, DUMMY, 3, 64, 64, 64.0, 63, NULL, DUMMY))):
        assert f(*args, None) == -1, msg
        err = L.last_error()
        assert err.startswith("genpc_gather_colors_ragged: ") and msg in err, (msg, err)
    assert f(0, NULL, NULL, NULL, 3, 64, 64, 64.0, 63, NULL, NULL, None) == 1
    assert f(2, cast(ints(0, 0, 0)), NULL, NULL, 3, 64, 64, 64.0, 63, NULL, NULL, None) == 1


def test_the_exported_plan(L):
    def plan(c, off, res=64, ps=1, rate=3):
        out = (ctypes.c_longlong * 7)(*([-7] * 7))
        return L.lib.genpc_depth_prompt_ragged_plan(c, cast(off), res, ps, rate, cast(out)), tuple(out)
    fill = 5 * 12 + 2 * 5 * 64 * 64
    items = (5560 >> 10) + 5
    assert plan(5, ints(0, 1, 3, 260, 560, 5560)) == (1, (items, 4, 1, 0, -1, fill, fill * 4 + items * 16 + 5 * 32))
    rc, out = plan(3, ints(0, 300, 300, 5300))                 # the empty scan in the middle is refused by its number
    assert rc == 1 and out[:5] == (8, 4, 1, 1, 1)
    rc, one = plan(1, ints(0, 5000))
    assert rc == 1 and one[1:3] == (4, 1)                      # the launch count does not depend on c
    assert plan(0, None) == (1, (0, 0, 0, 0, -1, 0, 0))
    rc, out = plan(2, ints(0, 9, 5))
    assert rc == -1 and out == (0, 0, 0, 0, -1, 0, 0) and L.last_error() == "genpc_depth_prompt_ragged_plan: offsets must ascend"
    assert L.lib.genpc_depth_prompt_ragged_plan(1, cast(ints(0, 5)), 64, 1, 3, NULL) == -1


def cfg():
    return SimpleNamespace(device="cpu", fovy=49.1, res=64, cam_res=64, padding=0.15, rescale=True, point_size=1, mask_pixel_rate=3,
                           view_num=8, distance=1.6, downsample_num=10000, removal_radius=10000, generative_model="trellis",
                           dataset="redwood")


class DeviceOffsets(torch.Tensor):
    """Offsets that say they live on a device (no GPU here to put them on)."""
    is_cuda = True


def device_offsets(*v):
    return torch.tensor(v, dtype=torch.int32).as_subclass(DeviceOffsets)


def clouds(*sizes, w=3):
    return [torch.arange(n * w, dtype=torch.float32).reshape(n, w) for n in sizes]


def test_get_depths_refuses(L):
    from genpc_amd.DepthPrompting import DepthPrompting
    dp = DepthPrompting(cfg())
    f = dp.getDepths
    with pytest.raises(RuntimeError, match="getDepths: GPU tensors only"):
        f(clouds(5, 7))
    with pytest.raises(RuntimeError, match="getDepths: GPU tensors only"):
        f((torch.zeros(12, 3), [0, 5, 12]))
    with pytest.raises(TypeError, match=r"getDepths: clouds\[0\] must be torch.float32"):
        f([c.double() for c in clouds(5)])
    with pytest.raises(ValueError, match=r"getDepths: clouds\[1\] must be an \[N,3\] tensor"):
        f([torch.zeros(5, 3), torch.zeros(6, 2)])
    with pytest.raises(TypeError, match="getDepths: clouds is a list"):
        f(torch.zeros(5, 3))
    with pytest.raises(ValueError, match="getDepths: the offsets of clouds live on the host"):
        f((torch.zeros(12, 3), device_offsets(0, 5, 12)))
    with pytest.raises(ValueError, match="getDepths: flags is None or a list with one entry per scan"):
        f(clouds(5, 7), flags=["a"])
    with pytest.raises(ValueError, match="getDepths: rgbs is None, a packed"):
        f(clouds(5, 7), rgbs=clouds(5))
    with pytest.raises(ValueError, match=r"getDepths: rgbs\[1\] must be \[7,3\]"):
        f(clouds(5, 7), rgbs=clouds(5, 6))
    with pytest.raises(TypeError, match=r"getDepths: rgbs\[0\] must be torch.float32"):
        f(clouds(5, 7), rgbs=[c.double() for c in clouds(5, 7)])
    with pytest.raises(ValueError, match="getDepths: packed rgbs must be"):
        f(clouds(5, 7), rgbs=torch.zeros(11, 3))
    assert f([]) == []


def test_color_points_refuses(L):
    from genpc_amd.ScaleAdapter import ScaleAdapter
    f = ScaleAdapter(cfg()).colorPoints
    imgs = [torch.zeros(3, 64, 64), torch.zeros(3, 64, 64)]
    with pytest.raises(RuntimeError, match="colorPoints: GPU tensors only"):
        f(clouds(5, 7, w=2), imgs, scale=64)
    with pytest.raises(ValueError, match="colorPoints: one image per scan"):
        f(clouds(5, 7, w=2), imgs[:1], scale=64)
    with pytest.raises(ValueError, match=r"colorPoints: imgs must be \[2,3,H,W\]"):
        f(clouds(5, 7, w=2), torch.zeros(3, 3, 64, 64), scale=64)
    with pytest.raises(ValueError, match=r"colorPoints: uvs\[1\] must be an \[N,2\] tensor"):
        f([torch.zeros(5, 2), torch.zeros(7, 3)], imgs, scale=64)
    with pytest.raises(TypeError, match=r"colorPoints: uvs\[0\] must be torch.float32"):
        f([c.double() for c in clouds(5, 7, w=2)], imgs, scale=64)
    with pytest.raises(TypeError, match=r"colorPoints: imgs\[1\] must be torch.float32"):
        f(clouds(5, 7, w=2), [imgs[0], imgs[1].double()], scale=64)
    with pytest.raises(ValueError, match=r"colorPoints: imgs\[1\] must be \[3,H,W\] like imgs\[0\]"):
        f(clouds(5, 7, w=2), [imgs[0], torch.zeros(3, 32, 64)], scale=64)
    with pytest.raises(ValueError, match="colorPoints: the offsets of uvs live on the host"):
        f((torch.zeros(12, 2), device_offsets(0, 5, 12)), imgs, scale=64)
    with pytest.raises(ValueError, match="colorPoints: the offsets of uvs must ascend"):
        f((torch.zeros(12, 2), [0, 5, 11]), imgs, scale=64)
    with pytest.raises(TypeError, match="colorPoints: uvs is a list"):
        f(torch.zeros(5, 2), imgs, scale=64)
    assert f([], []) == []


def test_complete_scans_batched_refuses(L):
    from genpc_amd import pipeline
    assert pipeline.complete_scans_batched([]) == []
    with pytest.raises(ValueError, match=r"complete_scans_batched: jobs\[0\] must be"):
        pipeline.complete_scans_batched([(torch.zeros(5, 3),)])
