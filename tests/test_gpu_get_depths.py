"""DepthPrompting.getDepths against a loop of getDepth, and ScaleAdapter.colorPoints against a loop of colorPoint, on three
scans of 300, 2500 and 12000 points (seeded blobs on a sphere; the largest exceeds downsample_num = 10000 and goes through the
batched farthest-point sampling), view_num 64, res 64.  Everything bit for bit except depth_sums: the per-scan path sums in
float32 (torch), the batched one in float64, n 2^-22 relative; the decision margin |sum0 - sum1| > n 2^-22 max|sum| is asserted
on the inputs -- a failure, never a skip -- so the two paths cannot decide differently from rounding alone."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (300, 2500, 12000)
BITS = ("visible", "uv", "depth", "pixels", "sparse_img", "raw_depth", "hole_mask1", "hole_mask2")
FILES = ("raw_depth.png", "mask.png", "point_uv.npy", "viewpoint.npy", "camera.pth")


def blob_cloud(seed, n):
    """A few gaussian blobs pressed onto a sphere of radius 0.45: a surface with a front and a back from every viewpoint."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(5, 3))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    p = centres[rng.integers(0, 5, n)] + rng.normal(scale=0.35, size=(n, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    return (p * 0.45 * (1 + 0.02 * rng.normal(size=(n, 1)))).astype(np.float32)


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd.DepthPrompting import DepthPrompting
    from genpc_amd.ScaleAdapter import ScaleAdapter
    root = tmp_path_factory.mktemp("stage1")
    cfg = SimpleNamespace(output_path=str(root), device="cuda", fovy=49.1, res=64, cam_res=64, padding=0.15, rescale=True, point_size=1,
                          mask_pixel_rate=3, view_num=64, distance=1.6, downsample_num=10000, removal_radius=10000, inpainter="flux",
                          generative_model="trellis", dataset="redwood")
    dp = DepthPrompting(cfg)
    clouds = [torch.from_numpy(blob_cloud(31 + j, n)).cuda() for j, n in enumerate(SIZES)]
    g = torch.Generator().manual_seed(3)
    rgbs = [torch.rand(c.shape, generator=g).cuda() for c in clouds]
    # the per-scan path, computed once and left unchanged; scan 1 writes its files
    single = [dp.getDepth(clouds[j], "single" if j == 1 else None, rgbs[j]) for j in range(3)]
    return dict(torch=torch, cfg=cfg, dp=dp, sa=ScaleAdapter(cfg), clouds=clouds, rgbs=rgbs, single=single, root=root)


def test_get_depths_against_get_depth(env):
    torch, dp, single = env["torch"], env["dp"], env["single"]
    got = dp.getDepths(env["clouds"], flags=[None, "batched", None], rgbs=env["rgbs"])
    assert len(got) == 3
    for j, n in enumerate(SIZES):
        g, w, what = got[j], single[j], "scan %d" % j
        assert set(g) == set(w), what
        s0, s1 = g["depth_sums"]
        big = max(abs(s0), abs(s1))
        print("%s: n %d, view %d, opposite %s, sums %.17g %.17g (per scan: %.9g %.9g), margin %.3e against %.3e"
              % (what, n, g["view_index"], g["used_opposite"], s0, s1, w["depth_sums"][0], w["depth_sums"][1], abs(s0 - s1), n * 2.0 ** -22 * big))
        assert abs(s0 - s1) > n * 2.0 ** -22 * big, what                       # the margin: a condition on the inputs
        assert g["view_index"] == w["view_index"] and g["used_opposite"] == w["used_opposite"], what
        for r in range(2):
            assert abs(g["depth_sums"][r] - w["depth_sums"][r]) <= n * 2.0 ** -22 * abs(g["depth_sums"][r]), (what, r)
        for k in BITS:
            assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape, (what, k)
            assert g[k].cpu().numpy().tobytes() == w[k].cpu().numpy().tobytes(), (what, k)
        assert int(g["visible"].sum()) > 0, what
    assert len(dp.point_uvs) == 3 and torch.equal(dp.point_uvs[2], got[2]["uv"])
    # packed input, white colours: the same geometry
    packed = dp.getDepths((torch.cat(env["clouds"]), [0, 300, 2800, 14800]))
    for j in range(3):
        for k in ("visible", "uv", "depth", "pixels", "raw_depth"):
            assert torch.equal(packed[j][k], got[j][k]), (j, k)
    # the stage-1 files of scan 1 are getDepth's, byte for byte
    for f in FILES:
        a, b = os.path.join(env["root"], "single", f), os.path.join(env["root"], "batched", f)
        assert os.path.exists(a) and os.path.exists(b), f
        with open(a, "rb") as fa, open(b, "rb") as fb:
            assert fa.read() == fb.read(), f


def test_color_points_against_color_point(env):
    torch, sa, single = env["torch"], env["sa"], env["single"]
    g = torch.Generator().manual_seed(9)
    imgs = [torch.rand(3, 1024, 1024, generator=g).cuda() for _ in range(3)]
    got = sa.colorPoints([s["uv"] for s in single], imgs)
    for j in range(3):
        want = sa.colorPoint(single[j]["uv"], imgs[j])
        assert got[j].dtype == want.dtype and torch.equal(got[j], want), j
