"""pipeline.complete_scans_batched against complete_scan(overlap=False) per scan, on the three small scans of
tests/test_gpu_reg_scans.py (the same construction), with a ground truth each.  Stage 1 and the point colours bit for bit; reg
to the bars tests/test_gpu_reg_scans.py holds reg_tensors_scans to (its margin on the coarse sweep asserted first, as a
condition on the fixture); the fused clouds hold the same points; the metric within 1e-6."""
import numpy as np
import pytest

from test_gpu_coarse_sweeps import SCANS, box_surface, scan
from test_gpu_reg_scans import assert_margin, same_scan

pytestmark = pytest.mark.gpu

STAGE1 = ("visible", "uv", "depth", "pixels", "sparse_img", "sparse_depth", "hole_mask1", "hole_mask2", "point_colors")
METRIC_POINTS = 2048


@pytest.fixture(scope="module")
def rg():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib, reg_xyz
    return dict(torch=torch, R=reg_xyz, L=_lib)


def rows(t):
    a = t.cpu().numpy()
    return a[np.lexsort(a.T[::-1])]


def test_complete_scans_batched_against_complete_scan(rg):
    torch = rg["torch"]
    from genpc_amd import pipeline
    from genpc_amd.DepthPrompting import DepthPrompting
    cfg = pipeline.default_cfg("cuda", view_num=64)
    cfg.res = 64
    dp = DepthPrompting(cfg)
    g = torch.Generator().manual_seed(17)
    jobs = []
    for s in SCANS:
        src, tgt = scan(*s)
        gt = (box_surface(s[0] + 900, 4096, s[4]) / s[3]).astype(np.float32)          # the scan's own surface, sampled again
        jobs.append((torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), torch.rand(3, 1024, 1024, generator=g).cuda(),
                     torch.from_numpy(gt).cuda()))
    kw = dict(cfg=cfg, dp=dp, metric_points=METRIC_POINTS, cd_only_pose=True)
    want = [pipeline.complete_scan(*job, overlap=False, **kw) for job in jobs]
    got = pipeline.complete_scans_batched(jobs, **kw)
    assert len(got) == 3
    for j in range(3):
        what = "scan %d" % j
        g_, w = got[j], want[j]
        assert set(g_) == set(w), what
        assert g_["view"] == w["view"] and g_["used_opposite"] == w["used_opposite"], what
        for k in STAGE1:
            assert g_[k].dtype == w[k].dtype and g_[k].shape == w[k].shape, (what, k)
            assert g_[k].cpu().numpy().tobytes() == w[k].cpu().numpy().tobytes(), (what, k)
        assert np.array_equal(g_["reg"]["diff_transform"], w["reg"]["diff_transform"]), what
        n = assert_margin(rg, jobs[j][0], jobs[j][1], w["reg"]["diff_transform"], what)
        same_scan(rg, g_["reg"], w["reg"], n, what)
        assert g_["fused"].shape == w["fused"].shape and np.array_equal(rows(g_["fused"]), rows(w["fused"])), what
        assert g_["pred_metric_points"].shape == (METRIC_POINTS, 3) and g_["gt_metric_points"].shape == (METRIC_POINTS, 3)
        diff = (g_["metric"].double() - w["metric"].double()).abs().max().item()
        print("%s: metric %s against %s, largest difference %.3e" % (what, g_["metric"].tolist(), w["metric"].tolist(), diff))
        assert diff <= 1e-6, what
    # a job without a ground truth carries no metric
    one = pipeline.complete_scans_batched([jobs[0][:3]], **kw)
    assert "metric" not in one[0] and torch.equal(one[0]["uv"], got[0]["uv"])
