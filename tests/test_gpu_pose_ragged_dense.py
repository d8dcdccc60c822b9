"""The ragged alignment step and loop with their nearest neighbours from the all-pairs search (nn_search="dense":
csrc/nn_ragged_dense.hip) against the same calls on the grid search (nn_search="grid").  The two searches return the same bits and
every other launch of a step is the same launch, so loss, gradient, histories, transforms and parameters are compared for
EQUALITY -- no tolerance.  How near the grid path is to the oracle and to the per-scan loop is tests/test_gpu_pose_ragged_step.py's
and tests/test_gpu_pose_ragged_loop.py's matter."""
import numpy as np
import pytest

from pose_ragged_step_cases import FULL, PAIRS, RADIUS, SIZE, element
from test_gpu_geometry import _shape

pytestmark = pytest.mark.gpu

SIZES = ((700, 300), (257, 450), (64, 130))          # (complete, partial) of the loop's three scans


@pytest.fixture(scope="module")
def gp():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib
    from genpc_amd.optim_registration import diff_obj_pose as POSE
    return dict(torch=torch, POSE=POSE, L=_lib)


_ELEMENTS = {}


def _step(gp, ks, mask, coloured, nn_search):
    torch, POSE = gp["torch"], gp["POSE"]
    for k in ks:
        if k not in _ELEMENTS:
            _ELEMENTS[k] = element(k)
    els = [_ELEMENTS[k] for k in ks]
    dev = lambda name: [torch.from_numpy(np.array(x[name])).cuda() for x in els]      # noqa: E731
    kw = dict(vert_col=dev("ccol"), partial_col=dev("pcol")) if mask and coloured else {}
    if not mask:
        kw["mask_weight"] = 0.0
    loss, grad = POSE.pose_loss_grad_ragged(dev("complete"), torch.stack(dev("center")), torch.stack(dev("params")), dev("partial"),
                                            RADIUS, SIZE, nn_search=nn_search, **kw)
    assert gp["L"].lib.genpc_nn_ragged_tune(0) == 0          # the thread's mode is what it was
    return loss.cpu().numpy(), grad.cpu().numpy()


def _equal(what, a, b):
    for name, x, y in zip(("loss", "gradient"), a, b):
        assert np.isfinite(x).all(), what
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), "%s: the %s differs, by at most %.3e" % (what, name, np.abs(x - y).max())


def test_one_step_six_pairs_chamfer_only(gp):
    ks = tuple(range(len(PAIRS)))
    _equal("six pairs, Chamfer only", _step(gp, ks, False, False, "dense"), _step(gp, ks, False, False, "grid"))
    _equal("six pairs reversed, Chamfer only", _step(gp, ks[::-1], False, False, "dense"), _step(gp, ks[::-1], False, False, "grid"))


@pytest.mark.parametrize("blend", [1, 0], ids=["pulsar_blend", "coverage_splat"])
@pytest.mark.parametrize("coloured", [False, True], ids=["white", "coloured"])
def test_one_step_full_objective(gp, blend, coloured):
    prev = gp["L"].lib.genpc_render_tune(blend)
    try:
        _equal("five pairs, blend %d, coloured %s" % (blend, coloured), _step(gp, FULL, True, coloured, "dense"), _step(gp, FULL, True, coloured, "grid"))
    finally:
        gp["L"].lib.genpc_render_tune(prev)


@pytest.fixture(scope="module")
def scans(gp):
    torch = gp["torch"]
    C, P = [], []
    for j, (nc, np_) in enumerate(SIZES):
        complete, partial, _ = _shape(40 + j, max(nc, 4 * np_, 64))
        assert len(complete) >= nc and len(partial) >= np_
        C.append(torch.from_numpy(np.ascontiguousarray(complete[:nc])).cuda())
        P.append(torch.from_numpy(np.ascontiguousarray(partial[:np_])).cuda())
    return C, P


def _loop(gp, scans, nn_search, cd_only=False):
    T, h, bp = gp["POSE"].object_pose_optimization_scans(scans[0], scans[1], radius=RADIUS, lr=0.01, iters=20, render_size=SIZE, cam_bias_num=4,
                                                         return_history=True, cd_only=cd_only, nn_search=nn_search)
    assert gp["L"].lib.genpc_nn_ragged_tune(0) == 0
    assert len(T) == len(h) == len(bp) == len(SIZES) and h[0].shape == (4, 21)
    return np.stack(T), np.stack(h), np.stack(bp)


def _same_loop(what, a, b):
    for name, x, y in zip(("transforms", "histories", "parameters"), a, b):
        assert np.isfinite(x).all(), what
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), "%s: the %s differ, by at most %.3e" % (what, name, np.abs(x - y).max())


@pytest.mark.parametrize("cd_only", [False, True], ids=["full", "chamfer_only"])
def test_the_loop_three_sizes(gp, scans, cd_only):
    d = _loop(gp, scans, "dense", cd_only)
    g = _loop(gp, scans, "grid", cd_only)
    _same_loop("dense against grid", d, g)
    _same_loop("dense again", _loop(gp, scans, "dense", cd_only), d)
    assert (d[1][:, :, -1] < d[1][:, :, 0]).any()          # (the loop did something)


def test_workspace_released_first_and_slots_across_modes(gp, scans):
    """The dense loop takes neither grid slot: it must run on a workspace that holds nothing, and a grid call behind it must find
    (and size) its slots itself."""
    torch, L = gp["torch"], gp["L"]
    g0 = _loop(gp, scans, "grid")
    torch.cuda.synchronize()
    assert L.lib.genpc_release_workspace() == 1
    d = _loop(gp, scans, "dense")
    g1 = _loop(gp, scans, "grid")
    _same_loop("dense on a released workspace", d, g0)
    _same_loop("grid behind the dense call", g1, g0)
    two = (scans[0][:2], scans[1][:2])                      # another number of elements through the same slots, in both modes
    _same_loop("two scans", _loop2(gp, two, "dense"), _loop2(gp, two, "grid"))
    _same_loop("three scans again", _loop(gp, scans, "dense"), g0)


def _loop2(gp, scans, nn_search):
    T, h, bp = gp["POSE"].object_pose_optimization_scans(scans[0], scans[1], radius=RADIUS, lr=0.01, iters=20, render_size=SIZE, cam_bias_num=4,
                                                         return_history=True, nn_search=nn_search)
    return np.stack(T), np.stack(h), np.stack(bp)


def test_refusals_by_name(gp):
    """The dense plan's refusals are the pose call's, before anything is enqueued: tiny buffers, tables that claim far more."""
    import ctypes
    torch, L = gp["torch"], gp["L"]
    x = torch.rand(8, 3).cuda()
    out = torch.zeros(2, 16).cuda()
    z = ctypes.c_void_p(0)
    big = ctypes.cast((ctypes.c_int * 2)(0, (1 << 20) + 1), ctypes.c_void_p)
    small = ctypes.cast((ctypes.c_int * 2)(0, 4), ctypes.c_void_p)
    half = ctypes.cast((ctypes.c_int * 2)(0, (1 << 18) + 1), ctypes.c_void_p)
    assert L.lib.genpc_nn_ragged_tune(1) == 0
    try:
        rc = L.lib.genpc_pose_optimize_ragged(1, big, small, L.ptr(x), z, L.ptr(x), z, 0.01, 2, 1, 0.0, 0, 0.0, L.ptr(out), z, z, z)
        assert rc == -1 and "genpc_pose_optimize_ragged" in L.last_error() and "2^20" in L.last_error()
        rc = L.lib.genpc_pose_loss_grad_ragged(1, half, half, L.ptr(x), z, L.ptr(x), L.ptr(x), L.ptr(x), z, 3.0, 0.001, 0.0, 0.0, 0, L.ptr(out), L.ptr(out), z)
        assert rc == -1 and "genpc_pose_loss_grad_ragged" in L.last_error() and "2^36" in L.last_error()
    finally:
        L.lib.genpc_nn_ragged_tune(0)
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0
