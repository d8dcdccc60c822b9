"""The densification of the partial scan (genpc_amd/utils/dataUtils.py: linear_interpolation, random_add_points,
xyz2xyzrgb) on the GPU, against tests/golden/ref_py_interp.npz: the reference's own linear_interpolation (scipy's
KD-tree) for every one of the 1000 recorded queries, and the float64 restatement of random_add_points."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dz(golden):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd.utils import dataUtils
    from genpc_amd.knn import knn_query
    return dict(torch=torch, D=dataUtils, knn=knn_query, fx=golden("ref_py_interp.npz"))


@pytest.mark.parametrize("k", [2, 5])
def test_linear_interpolation_is_the_references(dz, k):
    torch, fx = dz["torch"], dz["fx"]
    points, queries = fx["interp_points"], fx["interp_queries"]
    _, idx = dz["knn"](torch.from_numpy(queries.astype(np.float32)).cuda(), torch.from_numpy(points).cuda(), k)
    idx = idx.cpu().numpy()
    # the same neighbour SETS as scipy for every query (here even the same order: no query is left out)
    np.testing.assert_array_equal(np.sort(idx, axis=1), np.sort(fx["interp_idx6"][:, :k], axis=1))
    np.testing.assert_array_equal(idx, fx["interp_idx6"][:, :k])
    out = dz["D"].linear_interpolation(points, queries, k=k)
    assert isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == (1000, 3)
    np.testing.assert_allclose(out, fx["interp_k%d" % k], rtol=1e-12, atol=0)
    # GPU tensors in, GPU tensor out: the same numbers
    tout = dz["D"].linear_interpolation(torch.from_numpy(points).cuda(), torch.from_numpy(queries).cuda(), k=k)
    assert tout.is_cuda and tout.dtype == torch.float64
    np.testing.assert_allclose(tout.cpu().numpy(), fx["interp_k%d" % k], rtol=1e-9, atol=1e-12)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        dz["D"].linear_interpolation(torch.from_numpy(points), torch.from_numpy(queries), k=k)


def test_random_add_points_is_the_restatement(dz):
    torch, fx = dz["torch"], dz["fx"]
    coords = fx["add_coords"]
    out = dz["D"].random_add_points(coords)
    assert isinstance(out, np.ndarray) and out.dtype == np.float64
    n_in = len(out) - len(coords)
    np.testing.assert_array_equal(out[n_in:], coords.astype(np.float64))          # `inside` first, then coords
    c64 = coords.astype(np.float64)
    np.random.seed(0)
    cand = np.random.uniform(low=c64.min(axis=0), high=c64.max(axis=0), size=(100000, 3))
    # the kept candidates, in the candidates' order: every row of `inside` is matched in one forward pass
    keep = np.zeros(len(cand), bool)
    at = 0
    for row in out[:n_in]:
        while at < len(cand) and not np.array_equal(cand[at], row):
            at += 1
        assert at < len(cand), "a row of `inside` is not a candidate, or out of order"
        keep[at] = True
        at += 1
    np.testing.assert_array_equal(keep[:4000], fx["add_keep"])
    tout = dz["D"].random_add_points(torch.from_numpy(coords).cuda())
    assert tout.is_cuda and tout.dtype == torch.float64
    np.testing.assert_array_equal(tout.cpu().numpy(), out)


def test_xyz2xyzrgb_round_trip(dz, tmp_path):
    D = dz["D"]
    pts = dz["fx"]["add_coords"][:300]
    path = os.path.join(str(tmp_path), "partial.ply")
    D.save_ply_xyzrgb(pts, None, path)
    lo, hi = 0.5, 0.5 + D.C0 / 255.0
    coords, rgb = D.xyz2xyzrgb(path, add_point_type="random")
    assert coords.shape[1] == 3 and coords.shape[0] > 300 and rgb.shape == coords.shape
    np.testing.assert_array_equal(coords[-300:], pts.astype(np.float64))          # the original points are retained
    assert rgb.min() >= lo and rgb.max() <= hi
    near = np.sqrt(((coords[:-300, None, :] - pts[None].astype(np.float64)) ** 2).sum(axis=2)).min(axis=1)
    assert (near < 0.01).all()
    coords, rgb = D.xyz2xyzrgb(path, add_point_type="linear", add_num_points=200)
    assert coords.shape == (200, 3) and rgb.shape == (200, 3) and rgb.min() >= lo and rgb.max() <= hi
    assert (coords >= pts.min(axis=0) - 1e-6).all() and (coords <= pts.max(axis=0) + 1e-6).all()
    coords, rgb = D.xyz2xyzrgb(path, add_point_type="none")
    np.testing.assert_array_equal(coords, pts)
    assert rgb.shape == (300, 3)
