"""reg over a list of scans (reg_xyz.reg_tensors_scans, reg_xyz.reg_scans) against reg_tensors / reg on each scan alone.

Every stage but the coarse score is compared bit for bit.  The coarse score is mean(sqrt(d1)) + w mean(sqrt(d2)) summed in
another order by the ragged sweep: tests/test_gpu_coarse_sweeps.py derives bound(n) = 2 (n - 1) 2^-24 relative for clouds of
at most n points, and its condition on the inputs -- best and second-best score of the single-scan sweep more than twice the
bound apart, so the argmin cannot flip -- is asserted here first, as a condition on the fixture and never as a skip.  The
down-sampled targets stay under 6180 points, where every ICP takes the one-workgroup plan and the ragged ICP returns the
single call's bits (asserted through genpc_icp_plan)."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import write_glb
from test_gpu_coarse_sweeps import SCANS, bound, scan
from test_gpu_mesh_sample import _ellipsoid_mesh

pytestmark = pytest.mark.gpu

BITS = ("coarse_transformation", "best_scales_transformation", "best_transformation_xyz")


@pytest.fixture(scope="module")
def rg():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib, reg_xyz
    return dict(torch=torch, R=reg_xyz, L=_lib)


def one_workgroup(rg, nt):
    out = (ctypes.c_int * 3)()
    assert rg["L"].lib.genpc_icp_plan(int(nt), ctypes.cast(out, ctypes.c_void_p)) == 1
    return out[0] == 1


def assert_margin(rg, partial, complete, diff_transform, what):
    """reg_tensors' own coarse stage on one scan, every candidate scored: the fixture's margin and the ICP plan."""
    torch, R = rg["torch"], rg["R"]
    source = R._apply(diff_transform, partial.contiguous().float())
    target, _, _ = R.normalize_numpy(complete.contiguous().float(), range=0.5)
    sd, td = R.voxel_down_sample(source, 0.03), R.voxel_down_sample(target, 0.03)
    n = max(int(sd.shape[0]), int(td.shape[0]))
    assert int(td.shape[0]) < 6180 and one_workgroup(rg, td.shape[0]), (what, td.shape)
    T = R.icp_with_scaling(sd, td, np.linspace(1.5, 0.8, 11), 0.075)
    inv = torch.as_tensor(np.linalg.inv(T), device=sd.device)
    tk = (td.double() @ inv[:, :3, :3].transpose(1, 2) + inv[:, None, :3, 3]).float().contiguous()
    cd = R._partial_cd_scores(sd.float()[None].expand(11, -1, -1).contiguous(), tk, 0.5).cpu().numpy().astype(np.float64)
    two = np.sort(cd)[:2]
    gap = (two[1] - two[0]) / two[0]
    print("%s: %d / %d points after the 0.03 grid, best %.8g second %.8g, relative gap %.3e, twice the bound %.3e"
          % (what, sd.shape[0], td.shape[0], two[0], two[1], gap, 2 * bound(n)))
    assert gap > 2 * bound(n), what
    return n


def same_scan(rg, got, want, n, what, pose=False):
    torch = rg["torch"]
    assert set(got) == set(want), what
    assert got["best_scale"] == want["best_scale"], what
    for k in BITS + ("diff_transform",):
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k)
    for k in ("source", "target"):
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (what, k)
    assert got["xyz_loss"] == want["xyz_loss"], what
    rel = abs(got["coarse_loss"] - want["coarse_loss"]) / want["coarse_loss"]
    print("%s: coarse_loss differs by %.3e relative (bound %.3e)" % (what, rel, bound(n)))
    assert rel <= bound(n), what


@pytest.fixture(scope="module")
def three(rg):
    """The three scans on the device and reg_tensors on each alone, identity and given pose -- computed once, left unchanged."""
    torch, R = rg["torch"], rg["R"]
    raw = [scan(*s) for s in SCANS]
    partials = [torch.from_numpy(s).cuda() for s, _ in raw]
    completes = [torch.from_numpy(t).cuda() for _, t in raw]
    kw = dict(generative_model="trellis", reg_fine_xyz=True)
    given = []
    for j in range(3):                                   # small rigid motions, none the identity
        T = np.eye(4)
        a = 0.02 * (j + 1)
        T[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        T[:3, 3] = [0.004 * (j + 1), -0.003, 0.002 * j]
        given.append(T)
    single = [R.reg_tensors(partials[j], completes[j], diff_init=False, **kw) for j in range(3)]
    single_given = [R.reg_tensors(partials[j], completes[j], diff_init=True, diff_transform=given[j], **kw) for j in range(3)]
    return dict(partials=partials, completes=completes, kw=kw, given=given, single=single, single_given=single_given)


def test_three_scans_identity_pose(rg, three):
    R = rg["R"]
    ns = [assert_margin(rg, three["partials"][j], three["completes"][j], np.eye(4), "scan %d" % j) for j in range(3)]
    got = R.reg_tensors_scans(three["partials"], three["completes"], diff_init=False, **three["kw"])
    assert len(got) == 3
    for j in range(3):
        same_scan(rg, got[j], three["single"][j], ns[j], "scan %d" % j)
        assert got[j]["source_col"] is None and got[j]["target_col"] is None
    assert len({g["best_scale"] for g in got}) >= 2, "the scans do not all share one best scale"
    # a one-scan list is the three-scan list's entry
    one = R.reg_tensors_scans([three["partials"][1]], [three["completes"][1]], diff_init=False, **three["kw"])
    assert len(one) == 1
    same_scan(rg, one[0], three["single"][1], ns[1], "scan 1 alone")
    for k in BITS:
        assert np.array_equal(one[0][k], got[1][k]), k
    assert one[0]["coarse_loss"] == got[1]["coarse_loss"] or abs(one[0]["coarse_loss"] - got[1]["coarse_loss"]) <= bound(ns[1]) * got[1]["coarse_loss"]
    assert R.reg_tensors_scans([], [], diff_init=False, **three["kw"]) == []


def test_three_scans_given_poses(rg, three):
    R = rg["R"]
    ns = [assert_margin(rg, three["partials"][j], three["completes"][j], three["given"][j], "scan %d, given pose" % j) for j in range(3)]
    got = R.reg_tensors_scans(three["partials"], three["completes"], diff_init=True, diff_transforms=three["given"], **three["kw"])
    for j in range(3):
        same_scan(rg, got[j], three["single_given"][j], ns[j], "scan %d, given pose" % j)
        assert not np.array_equal(got[j]["diff_transform"], np.eye(4))
        assert not np.array_equal(got[j]["coarse_transformation"], three["single"][j]["coarse_transformation"])


def test_pose_initialisation_per_scan(rg):
    """diff_init=True: the grids at pose_voxel come from one ragged call (one scan with colours, one without), the alignment loop
    runs per scan on the same bits as reg_tensors', and the loop repeats bit for bit (tests/test_gpu_determinism.py)."""
    torch, R = rg["torch"], rg["R"]
    raw = [scan(21, 4000, 3000, 1.1, 0.95), scan(22, 5000, 3500, 0.97, 1.0)]
    partials = [torch.from_numpy(s).cuda() for s, _ in raw]
    completes = [torch.from_numpy(t).cuda() for _, t in raw]
    g = torch.Generator().manual_seed(5)
    pcols = [torch.rand(partials[0].shape, generator=g).cuda(), None]
    ccols = [torch.rand(completes[0].shape, generator=g).cuda(), None]
    kw = dict(generative_model="trellis", diff_init=True, cd_only_pose=True)
    got = R.reg_tensors_scans(partials, completes, partial_cols=pcols, complete_cols=ccols, **kw)
    for j in range(2):
        want = R.reg_tensors(partials[j], completes[j], partial_col=pcols[j], complete_col=ccols[j], **kw)
        assert got[j]["diff_transform"].dtype == np.float64 and got[j]["diff_transform"].shape == (4, 4)
        assert np.array_equal(got[j]["diff_transform"], want["diff_transform"]), j
        assert not np.array_equal(want["diff_transform"], np.eye(4))
        assert (got[j]["source_col"] is None) == (pcols[j] is None)
        if pcols[j] is not None:
            assert torch.equal(got[j]["source_col"], pcols[j]) and torch.equal(got[j]["target_col"], ccols[j])


FLAGS = ("00042", "00043")


@pytest.fixture(scope="module")
def stage2(rg, tmp_path_factory):
    """A stage-2 directory of two flags (meshes of different face counts, partial clouds of different sizes) and reg() on each
    flag alone with seed 7 -- the reference, computed once."""
    torch, R = rg["torch"], rg["R"]
    from genpc_amd.utils import dataUtils as D, mesh_io as M
    root = tmp_path_factory.mktemp("stage2")
    cfg = SimpleNamespace(output_path=str(root), device="cuda", generative_model="trellis", dataset="redwood")
    glbs = []
    for j, flag in enumerate(FLAGS):
        base = root / flag
        os.makedirs(base)
        verts, faces, cols = _ellipsoid_mesh(*((48, 24), (40, 20))[j])
        glb = str(base / (flag + "_trellis.glb"))
        write_glb(glb, verts, faces, cols, indices_u16=True)
        glbs.append(glb)
        # the observed partial cloud: the mesh's front half, at 0.88 scale and slightly moved, with the mesh's colours
        pts, pcols = M.glb2point_gpu(glb, num_points=(6000, 5000)[j], seed=5 + j)
        pts, pcols = pts.cpu().numpy(), pcols.cpu().numpy()
        front = pts[:, 2] > -0.02
        partial = (pts[front] * 0.88 + np.array([0.015, -0.01, 0.01])).astype(np.float32)
        D.save_ply_xyzrgb(partial, pcols[front], str(base / "color_point.ply"))
    assert len({M.load_glb(g)[1].shape[0] for g in glbs}) == 2
    cwd = os.getcwd()
    os.chdir(str(root))                  # reg's pose initialisation drops its side-effect files into the working directory
    try:
        single, blobs = [], []
        for flag in FLAGS:
            out = R.reg(cfg, flag, seed=7)
            with open(out["fused_path"], "rb") as f:
                blobs.append(f.read())
            os.remove(out["fused_path"])
            single.append(out)
        for f in ("partial.png", "partial_mask.png", "final_transform.npy"):
            os.remove(f)
    finally:
        os.chdir(cwd)
    return dict(cfg=cfg, root=root, glbs=glbs, single=single, blobs=blobs)


def test_reg_scans_against_reg(rg, stage2):
    torch, R = rg["torch"], rg["R"]
    from genpc_amd.utils import dataUtils as D, mesh_io as M
    cfg, single = stage2["cfg"], stage2["single"]
    cwd = os.getcwd()
    os.chdir(str(stage2["root"]))
    try:
        runs, files = [], []
        for _ in range(2):
            runs.append(R.reg_scans(cfg, list(FLAGS), seed=7))
            blobs = []
            for o in runs[-1]:
                with open(o["fused_path"], "rb") as f:
                    blobs.append(f.read())
            files.append(blobs)
        left = sorted(os.listdir("."))
    finally:
        os.chdir(cwd)
    assert files[0] == files[1] and all(len(b) > 10000 * 27 for b in files[0])          # two runs write byte-identical files
    assert not {"partial.png", "partial_mask.png", "final_transform.npy"} & set(left), left
    got = runs[0]
    assert len(got) == 2
    for j, flag in enumerate(FLAGS):
        what = "flag %s" % flag
        sxyz, _ = D.read_ply(f"{cfg.output_path}/{flag}/color_point.ply")
        txyz, tcol = M.glb2point_gpu(stage2["glbs"][j], num_points=163840, seed=7)
        assert np.array_equal(got[j]["diff_transform"], single[j]["diff_transform"]), what          # (the pose needs no margin)
        assert_margin(rg, torch.as_tensor(sxyz, dtype=torch.float32, device="cuda"), txyz, single[j]["diff_transform"], what)
        for k in ("source", "target", "target_col", "source_col"):
            assert torch.equal(got[j][k], single[j][k]), (what, k)
        assert got[j]["target"].shape == (163840, 3) and torch.equal(got[j]["target_col"], tcol)
        assert got[j]["fused_path"] == f"{cfg.output_path}/{flag}/{flag}_fused.ply" and os.path.exists(got[j]["fused_path"])
        back, back_col = D.read_ply(got[j]["fused_path"])
        assert back.shape == tuple(got[j]["fused"].shape) and back_col is not None and back_col.shape == back.shape
        np.testing.assert_array_equal(back.astype(np.float32), got[j]["fused"].cpu().numpy())
    # the fused clouds are fuse_scans on reg's own aligned clouds, bit for bit
    again = R.fuse_scans([o["source"] for o in single], [o["target"] for o in single], num_points=20000, distance_threshold=0.0001,
                         std_ratio=2.5, source_cols=[o["source_col"] for o in single], target_cols=[o["target_col"] for o in single])
    for j in range(2):
        assert torch.equal(got[j]["fused"], again[j][0]) and torch.equal(got[j]["fused_col"], again[j][1]), j
    # ... and reg's own fused cloud whenever no point's k-NN mean lies within 1e-12 relative of its threshold
    for j in range(2):
        o = single[j]
        pre = R.fuse(o["source"], o["target"], num_points=20000, distance_threshold=0.0001, std_ratio=None,
                     source_col=o["source_col"], target_col=o["target_col"])[0]
        _, _, stats, _ = R.remove_noise_from_point_clouds([pre], std_ratio=2.5, return_stats=True)
        thr = float(stats[0, 2].item())
        means = R.knn_mean_distance_ragged([pre])[0].double()
        margin = float(((means - thr).abs() / thr).min().item())
        print("flag %s: the closest k-NN mean lies %.3e relative from the threshold" % (FLAGS[j], margin))
        if margin > 1e-12:
            assert torch.equal(got[j]["fused"], o["fused"]) and torch.equal(got[j]["fused_col"], o["fused_col"]), j
            assert files[0][j] == stage2["blobs"][j]
