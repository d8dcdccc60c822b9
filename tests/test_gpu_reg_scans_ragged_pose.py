"""reg_tensors_scans(..., ragged_pose=True): the scans that need a pose go through ONE object_pose_optimization_scans call on the
grids at pose_voxel.  This checks the WIRING: the full objective's 200 steps are not comparable between the per-scan and the
ragged path beyond the first steps (tests/test_gpu_geometry.py test_pose_loop_batched_equals_singles says why: the loss jumps by
100 / P when a soft-mask pixel saturates), so what the switch returns is compared with what the test itself gets from
object_pose_optimization_scans on the same grids -- which rests on the ragged loop repeating bit for bit
(tests/test_gpu_pose_ragged_loop.py)."""
import numpy as np
import pytest

from test_gpu_coarse_sweeps import scan

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rg():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import reg_xyz
    from genpc_amd.optim_registration import diff_obj_pose as POSE
    return dict(torch=torch, R=reg_xyz, POSE=POSE)


@pytest.fixture(scope="module")
def two(rg):
    torch = rg["torch"]
    raw = [scan(21, 4000, 3000, 1.1, 0.95), scan(22, 5000, 3500, 0.97, 1.0)]
    partials = [torch.from_numpy(s).cuda() for s, _ in raw]
    completes = [torch.from_numpy(t).cuda() for _, t in raw]
    g = torch.Generator().manual_seed(5)
    pcols = [torch.rand(partials[0].shape, generator=g).cuda(), None]          # one scan with colours, one without
    ccols = [torch.rand(completes[0].shape, generator=g).cuda(), None]
    return dict(partials=partials, completes=completes, pcols=pcols, ccols=ccols)


def test_given_poses_need_no_loop(rg, two, monkeypatch):
    """Every diff_transforms[j] given: the switch changes nothing and the pose is never called."""
    R, POSE = rg["R"], rg["POSE"]
    given = []
    for j in range(2):
        T = np.eye(4)
        a = 0.02 * (j + 1)
        T[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        T[:3, 3] = [0.004 * (j + 1), -0.003, 0.002 * j]
        given.append(T)
    kw = dict(generative_model="trellis", diff_init=True, diff_transforms=given, partial_cols=two["pcols"], complete_cols=two["ccols"])
    want = R.reg_tensors_scans(two["partials"], two["completes"], **kw)

    def never(*a, **k):
        raise AssertionError("the pose was called although every transform is given")
    monkeypatch.setattr(POSE, "object_pose_optimization_scans", never)
    monkeypatch.setattr(POSE, "object_pose_optimization", never)
    got = R.reg_tensors_scans(two["partials"], two["completes"], ragged_pose=True, **kw)
    for j in range(2):
        assert set(got[j]) == set(want[j])
        for k in ("diff_transform", "coarse_transformation"):
            assert np.array_equal(got[j][k], want[j][k]), (j, k)
        assert got[j]["best_scale"] == want[j]["best_scale"] and got[j]["coarse_loss"] == want[j]["coarse_loss"]
        for k in ("source", "target"):
            assert rg["torch"].equal(got[j][k], want[j][k]), (j, k)


@pytest.mark.parametrize("cd_only", [True, False], ids=["chamfer_only", "full_objective"])
def test_the_switch_calls_the_ragged_loop_on_the_pose_grids(rg, two, cd_only):
    torch, R, POSE = rg["torch"], rg["R"], rg["POSE"]
    kw = dict(generative_model="trellis", diff_init=True, cd_only_pose=cd_only)
    got = R.reg_tensors_scans(two["partials"], two["completes"], partial_cols=two["pcols"], complete_cols=two["ccols"], ragged_pose=True, **kw)
    # the same grids, by the same helper, and the ragged loop on them with reg's hyper-parameters
    down, dcol = R._voxel_grids(two["completes"] + two["partials"], 0.02, two["ccols"] + two["pcols"])
    assert len({int(d.shape[0]) for d in down}) == 4, [d.shape for d in down]          # four different sizes: a ragged call
    Ts = POSE.object_pose_optimization_scans(down[:2], down[2:], radius=0.02, lr=0.01, iters=200, render_size=224, cd_only=cd_only,
                                             complete_cols=dcol[:2], partial_cols=dcol[2:])
    for j in range(2):
        d = got[j]["diff_transform"]
        assert d.dtype == np.float64 and d.shape == (4, 4) and not np.array_equal(d, np.eye(4))
        assert np.array_equal(d, np.linalg.inv(Ts[j].astype(np.float64))), j
        assert (got[j]["source_col"] is None) == (two["pcols"][j] is None)
    # the default is the per-scan path: Chamfer-only, the two paths agree to what their summation orders allow
    if cd_only:
        per_scan = R.reg_tensors_scans(two["partials"], two["completes"], partial_cols=two["pcols"], complete_cols=two["ccols"], **kw)
        for j in range(2):
            dev = np.abs(per_scan[j]["diff_transform"] - got[j]["diff_transform"]).max()
            print("scan %d: per-scan and ragged pose differ by %.3e (Chamfer-only, 200 steps)" % (j, dev))
            assert np.isfinite(got[j]["diff_transform"]).all()
