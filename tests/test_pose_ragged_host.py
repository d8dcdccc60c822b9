"""The host side of the ragged alignment loop, without a GPU: the bindings, what the wrappers and the library refuse before any
GPU work, the chunking of a long list of scans, the `ragged_pose` switch of reg_tensors_scans / reg_scans, and the rules by
which the draws of tests/pose_ragged_step_cases.py were chosen."""
import ctypes
import inspect

import numpy as np
import pytest
import torch


def test_bindings_present_and_abi_unchanged():
    from genpc_amd import _lib
    for name, nargs in (("genpc_pose_optimize_ragged", 17), ("genpc_pose_loss_grad_ragged", 17), ("genpc_pose_ragged_plan", 9)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert getattr(_lib.lib, name) is not None
    assert _lib.ABI_VERSION == 28 and _lib.lib.genpc_abi_version() == 28


def _plan(L, nc, np_, starts, mask=1, size=224, radius=0.02, cus=256):
    coff = (ctypes.c_int * (len(nc) + 1))(*np.concatenate([[0], np.cumsum(nc)]).astype(int).tolist())
    poff = (ctypes.c_int * (len(np_) + 1))(*np.concatenate([[0], np.cumsum(np_)]).astype(int).tolist())
    out = (ctypes.c_int * 16)()
    rc = L.genpc_pose_ragged_plan(len(nc), ctypes.cast(coff, ctypes.c_void_p), ctypes.cast(poff, ctypes.c_void_p), starts, mask, size, radius, cus,
                                  ctypes.cast(out, ctypes.c_void_p))
    return rc, list(out)


def test_the_exported_plan():
    from genpc_amd import _lib
    L = _lib.lib
    rc, out = _plan(L, [4493] * 16, [886] * 16, 4)
    assert rc == 1
    assert out[0] == 64 and out[1] == 4493 and out[2] == 886 and out[3] == 18 and out[4] == 22 and out[5] == 1 and out[12] == 0
    assert out[7] == 1 and out[13] == 4 * 16 * 4493 and out[14] == 4 * 16 * 886
    rc, out = _plan(L, [10] * 97, [10] * 97, 4)
    assert rc == 1 and out[12] == 1          # too large: the entry points would refuse it
    rc, out = _plan(L, [10, 0], [10, 10], 4)
    assert rc == -1 and "genpc_pose_ragged_plan: scan 1 has an empty complete cloud" in _lib.last_error()
    assert L.genpc_pose_ragged_plan(0, None, None, 4, 1, 224, 0.02, 256, ctypes.cast((ctypes.c_int * 16)(), ctypes.c_void_p)) == 1


def test_the_library_refuses_before_any_gpu_work():
    """No device pointer is looked at by a refused call: the (never dereferenced) pointers here are not device memory."""
    from genpc_amd import _lib
    L = _lib.lib
    vp = ctypes.c_void_p
    z, fake = vp(0), vp(4096)

    def optimize(c, coff, poff, starts=4, iters=2, mask_weight=0.0, size=0, radius=0.0, complete=fake):
        co = (ctypes.c_int * len(coff))(*coff)
        po = (ctypes.c_int * len(poff))(*poff)
        return L.genpc_pose_optimize_ragged(c, ctypes.cast(co, vp), ctypes.cast(po, vp), complete, z, fake, z, 0.01, iters, starts, radius, size,
                                            mask_weight, fake, z, z, z)
    assert optimize(0, [0], [0]) == 1                                             # c = 0: nothing to do, nothing written
    assert L.genpc_pose_optimize_ragged(0, z, z, z, z, z, z, 0.01, 2, 4, 0.0, 0, 0.0, z, z, z, z) == 1
    for args, kw, why in (((-1, [0], [0]), {}, "negative number of scans"),
                          ((2, [1, 4, 8], [0, 4, 8]), {}, "offsets must start at 0"),
                          ((2, [0, 4, 8], [0, 5, 4]), {}, "offsets must ascend"),
                          ((2, [0, 4, 4], [0, 4, 8]), {}, "scan 1 has an empty complete cloud"),
                          ((3, [0, 4, 8, 9], [0, 0, 8, 9]), {}, "scan 0 has an empty partial cloud"),
                          ((97, list(range(98)), list(range(98))), {}, "more than 384 elements"),
                          ((2, [0, 4, 8], [0, 4, 8]), dict(starts=0), "starts must be at least 1"),
                          ((2, [0, 4, 8], [0, 4, 8]), dict(iters=-1), "iters at least 0"),
                          ((2, [0, 4, 8], [0, 4, 8]), dict(mask_weight=1.0, size=1, radius=0.02), "render_size > 1"),
                          ((2, [0, 4, 8], [0, 4, 8]), dict(mask_weight=1.0, size=64, radius=0.0), "positive radius"),
                          ((2, [0, 4, 8], [0, 4, 8]), dict(complete=z), "null pointer")):
        assert optimize(*args, **kw) == -1, why
        assert _lib.last_error().startswith("genpc_pose_optimize_ragged: ") and why in _lib.last_error(), (why, _lib.last_error())
    assert L.genpc_pose_optimize_ragged(2, z, z, fake, z, fake, z, 0.01, 2, 4, 0.0, 0, 0.0, fake, z, z, z) == -1
    assert "null offset table" in _lib.last_error()
    co = (ctypes.c_int * 3)(0, 4, 4)
    rc = L.genpc_pose_loss_grad_ragged(2, ctypes.cast(co, vp), ctypes.cast(co, vp), fake, z, fake, fake, fake, z, 3.0, 0.001, 0.0, 0.0, 0, fake, fake, z)
    assert rc == -1 and "genpc_pose_loss_grad_ragged: scan 1 has an empty complete cloud" in _lib.last_error()
    big = (ctypes.c_int * 386)(*range(386))
    rc = L.genpc_pose_loss_grad_ragged(385, ctypes.cast(big, vp), ctypes.cast(big, vp), fake, z, fake, fake, fake, z, 3.0, 0.001, 0.0, 0.0, 0, fake, fake, z)
    assert rc == -1 and "more than 384 elements" in _lib.last_error()


def test_chunks_of_a_long_list():
    from genpc_amd.optim_registration.diff_obj_pose import RAGGED_MAX_ELEMENTS, pose_scan_chunks
    assert RAGGED_MAX_ELEMENTS == 384
    assert pose_scan_chunks(97, 4) == [(0, 96), (96, 97)]
    assert pose_scan_chunks(96, 4) == [(0, 96)]
    assert pose_scan_chunks(16, 4) == [(0, 16)]
    assert pose_scan_chunks(0, 4) == []
    assert pose_scan_chunks(1000, 1) == [(0, 384), (384, 768), (768, 1000)]
    assert pose_scan_chunks(5, 384) == [(j, j + 1) for j in range(5)]
    assert pose_scan_chunks(300, 5) == [(0, 76), (76, 152), (152, 228), (228, 300)]          # 76 x 5 = 380 <= 384 < 77 x 5
    for s, k in ((97, 4), (1000, 1), (300, 5), (7, 100)):
        ch = pose_scan_chunks(s, k)
        assert ch[0][0] == 0 and ch[-1][1] == s and all(a[1] == b[0] for a, b in zip(ch, ch[1:])) and all((b - a) * k <= 384 and b > a for a, b in ch)
    with pytest.raises(ValueError):
        pose_scan_chunks(3, 385)
    with pytest.raises(ValueError):
        pose_scan_chunks(3, 0)


def test_wrappers_refuse_naming_the_scan():
    from genpc_amd.optim_registration import diff_obj_pose as POSE
    a, b = torch.rand(20, 3), torch.rand(10, 3)
    # CPU tensors: named by scan, for the list and for the packed form
    with pytest.raises(RuntimeError, match=r"GPU tensors only \(completes\[0\], scan 0"):
        POSE.object_pose_optimization_scans([a, a], [b, b])
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        POSE.object_pose_optimization_scans((torch.cat([a, a]), [0, 20, 40]), (torch.cat([b, b]), [0, 10, 20]))
    with pytest.raises(RuntimeError, match=r"GPU tensors only \(vert_pos\[0\], scan 0"):
        POSE.pose_loss_grad_ragged([a], torch.zeros(1, 3), torch.zeros(1, 10), [b], 0.02)
    with pytest.raises(TypeError):
        POSE.object_pose_optimization_scans(a, [b])


def test_wrapper_refusals_behind_the_cloud_check(monkeypatch):
    """List lengths, an empty cloud by number, colour lists: checked on meta-data alone.  The clouds' device check is switched off
    for this test (the tensors stay on the CPU and no library call is reached: every case raises first)."""
    from genpc_amd.optim_registration import diff_obj_pose as POSE

    def reached(*a, **k):
        raise AssertionError("a refused call reached the library")
    monkeypatch.setattr(POSE._lib, "on_device_of", reached)

    class Cuda(torch.Tensor):
        is_cuda = True

    def dev(t):
        return t.as_subclass(Cuda)
    a, b, e = dev(torch.rand(20, 3)), dev(torch.rand(10, 3)), dev(torch.rand(0, 3))
    with pytest.raises(ValueError, match=r"completes\[1\] must be an \[N,3\] tensor"):
        POSE.object_pose_optimization_scans([a, dev(torch.rand(20, 2))], [b, b])
    with pytest.raises(ValueError, match="2 complete clouds against 1 partial clouds"):
        POSE.object_pose_optimization_scans([a, a], [b])
    with pytest.raises(ValueError, match="scan 1 has an empty partial cloud"):
        POSE.object_pose_optimization_scans([a, a], [b, e])
    with pytest.raises(ValueError, match="scan 0 has an empty complete cloud"):
        POSE.object_pose_optimization_scans([e, a], [b, b])
    with pytest.raises(ValueError, match="complete_cols must be None or a list with one entry per scan"):
        POSE.object_pose_optimization_scans([a, a], [b, b], complete_cols=[torch.rand(20, 3)])
    with pytest.raises(ValueError, match=r"partial_cols\[1\] must have the shape of scan 1's cloud \(10, 3\)"):
        POSE.object_pose_optimization_scans([a, a], [b, b], partial_cols=[None, torch.rand(9, 3)])
    with pytest.raises(ValueError, match="1 complete clouds against 2 partial clouds"):
        POSE.pose_loss_grad_ragged([a], dev(torch.zeros(1, 3)), dev(torch.zeros(1, 10)), [b, b], 0.02)
    with pytest.raises(ValueError, match="scan 0 has an empty partial cloud"):
        POSE.pose_loss_grad_ragged([a], dev(torch.zeros(1, 3)), dev(torch.zeros(1, 10)), [e], 0.02)
    with pytest.raises(ValueError, match="pose_scan_chunks"):
        POSE.object_pose_optimization_scans([a], [b], cam_bias_num=385)


def test_reg_takes_the_switch():
    from genpc_amd import reg_xyz as R
    for fn in (R.reg_tensors_scans, R.reg_scans):
        p = inspect.signature(fn).parameters["ragged_pose"]
        assert p.default is False, fn.__name__          # the default keeps the per-scan path
    src = inspect.getsource(R.reg_scans)
    assert "ragged_pose=ragged_pose" in src and "object_pose_optimization_scans(" in src          # reg_scans hands the switch on
    assert "object_pose_optimization_scans(" in inspect.getsource(R.reg_tensors_scans)
    # nothing else may come in through **kwargs, the switch included where it does not belong
    with pytest.raises(TypeError):
        R.reg_tensors_scans([], [], ragged=True)
    assert R.reg_tensors_scans([], [], ragged_pose=True) == []


def test_the_chosen_draws_keep_their_rules(oracle):
    """tests/pose_ragged_step_cases.py: every pair's committed draw passes the rim rule and the conditioning rule, the first
    cloud drawn for pair (63, 257) does not (that pixel is why the table exists), and select() gives the committed table."""
    import pose_ragged_step_cases as C
    for k in range(len(C.PAIRS)):
        x = C.element(k)
        assert x["complete"].shape == (C.PAIRS[k][0], 3) and x["partial"].shape == (C.PAIRS[k][1], 3)
        if k in C.FULL:
            assert C.rim_margin(oracle, x) > C.kRim, k
        assert C.conditioning(oracle, k, x) < C.kCond, k
    assert C.rim_margin(oracle, C.element(1, 0)) < 1e-5
    assert C.select(oracle) == C.RESEED
