"""The ragged mesh sampler (csrc/mesh_sample_ragged.hip -> genpc_mesh_sample_ragged -> utils/mesh_io.sample_surfaces_gpu /
glb2points_gpu) against the numpy restatement of the sampler's definition (tests/mesh_sample_ref.py) and against
genpc_mesh_sample on each mesh alone.  Every comparison is bit for bit: points, faces, barycentric weights, colours, status."""
import numpy as np
import pytest

import mesh_sample_ref as R
from conftest import write_glb
from test_gpu_mesh_sample import _ellipsoid_mesh

pytestmark = pytest.mark.gpu

KEYS = ("points", "face", "bary", "colors")


def _ragged(meshes, counts, seeds):
    """One sample_surfaces_gpu's worth of library calls, status not judged -> a list of numpy dicts, one per mesh."""
    from genpc_amd.utils import mesh_io as M
    r = M._mesh_sample_ragged(meshes, counts, seeds, want_bary=True)
    soff, status = r["soff"], r["status"].cpu().numpy()
    out = []
    for j in range(len(soff) - 1):
        sl = slice(soff[j], soff[j + 1])
        out.append(dict(points=r["points"][sl].cpu().numpy(), face=r["face"][sl].cpu().numpy(), bary=r["bary"][sl].cpu().numpy(),
                        colors=None if r["colors"] is None else r["colors"][sl].cpu().numpy(), status=int(status[j])))
    return out


def _single(V, F, count, seed, C=None):
    from genpc_amd.utils import mesh_io as M
    r = M._mesh_sample(V, F, count, seed, colors=C, want_bary=True)
    w, cum = M.mesh_sample_weights(r["workspace"], r["nf"])
    return dict(points=r["points"].cpu().numpy(), face=r["face"].cpu().numpy(), bary=r["bary"].cpu().numpy(),
                colors=None if r["colors"] is None else r["colors"].cpu().numpy(), status=int(r["status"].item()), w=w, cum=cum)


def _same(got, want, what):
    assert got["status"] == want["status"] == 1, what
    for k in KEYS:
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
            np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (what, k))


def test_mixed_sizes_bit_for_bit():
    """One face, the scan boundaries (a lane holds 4 faces, a wave 256, a workgroup 1024) and more than one chunk, in one call
    and not in ascending order; counts with partial waves, a partial last workgroup and none at all; every seed different."""
    sizes = (1025, 1, 5000, 256, 2, 1024, 257, 255)
    counts = (4097, 63, 65, 0, 1, 64, 4097, 65)
    assert set(counts) == {0, 1, 63, 64, 65, 4097} and sorted(sizes) == [1, 2, 255, 256, 257, 1024, 1025, 5000]
    meshes = [R.grid_mesh(nf, seed=nf) for nf in sizes]
    seeds = [2000 + 7 * j for j in range(len(sizes))]
    got = _ragged(meshes, list(counts), seeds)
    for j, (V, F, C) in enumerate(meshes):
        what = "mesh %d (nf %d, count %d)" % (j, sizes[j], counts[j])
        assert got[j]["status"] == 1, what
        if counts[j] == 0:
            assert got[j]["points"].shape == (0, 3) and got[j]["face"].shape == (0,)
            continue
        want = R.sample(V, F, counts[j], seeds[j], colors=C)
        _same(got[j], want, what + " against the definition")
        alone = _single(V, F, counts[j], seeds[j], C)
        np.testing.assert_array_equal(alone["w"], want["w"])
        _same(got[j], alone, what + " against genpc_mesh_sample")
    assert len(np.unique(got[2]["face"])) > 16 and got[2]["face"].max() >= 1024          # (the second search level was used)


def _big_grid(nf, seed):
    """grid_mesh's jittered height field for millions of faces, without a Python loop."""
    rng = np.random.default_rng(seed)
    cols = 1024
    rows = (nf + 2 * cols - 1) // (2 * cols)
    gx, gy = np.meshgrid(np.arange(cols + 1, dtype=np.float64), np.arange(rows + 1, dtype=np.float64))
    V = np.stack([gx, gy, np.zeros_like(gx)], -1).reshape(-1, 3) + 0.2 * rng.standard_normal(((rows + 1) * (cols + 1), 3))
    a = (np.arange(rows)[:, None] * (cols + 1) + np.arange(cols)[None, :]).reshape(-1)
    F = np.stack([np.stack([a, a + 1, a + cols + 1], -1), np.stack([a + 1, a + cols + 2, a + cols + 1], -1)], 1).reshape(-1, 3)
    return V.astype(np.float32), F[:nf].astype(np.int32), rng.random(V.shape).astype(np.float32)


def test_a_mesh_over_2_21_faces_beside_a_small_one():
    """More than 2048 chunk sums: the unstaged chunk search, in the same launch as a 300-face mesh (staged)."""
    nf = (1 << 21) + 65536 + 1500
    big, small = _big_grid(nf, 3), R.grid_mesh(300, seed=4)
    assert big[1].shape == (nf, 3) and (nf + 1023) // 1024 > 2048
    got = _ragged([big, small], 4097, [91, 92])
    for j, (V, F, C) in enumerate((big, small)):
        alone = _single(V, F, 4097, 91 + j, C)
        _same(got[j], alone, "mesh %d against genpc_mesh_sample" % j)
    # (numpy weighs 2.1 million faces in well under a second: the single call's weights against the definition, and through
    # them the faces both calls drew)
    w, cum, bad = R.face_weights(big[0], big[1])
    alone = _single(big[0], big[1], 64, 91, big[2])
    assert not bad
    np.testing.assert_array_equal(alone["w"], w)
    np.testing.assert_array_equal(alone["cum"], cum)
    assert got[0]["face"].max() > 2048 * 1024          # (faces beyond the 2048th chunk were drawn)


def _bad_batch():
    meshes = [list(R.grid_mesh(600, seed=10 + j)) for j in range(7)]
    meshes[1][1] = meshes[1][1].copy()
    meshes[1][1][300, 1] = len(meshes[1][0])            # = nv_1: a vertex of mesh 2 stands there in the packed array
    meshes[2][1] = meshes[2][1].copy()
    meshes[2][1][599, 2] = -1
    meshes[3][0] = meshes[3][0].copy()
    meshes[3][0][int(meshes[3][1][17, 0]), 1] = np.nan
    meshes[4][1] = np.array([[3, 3, 4], [0, 0, 0], [7, 8, 7]], np.int32)          # every face degenerate
    V, F, C = meshes[6]
    meshes[6] = [np.concatenate([V, np.full((1, 3), np.nan, np.float32)]), F, np.concatenate([C, np.full((1, 3), 0.25, np.float32)])]
    return [tuple(m) for m in meshes]


def test_bad_meshes_in_one_call():
    """A bad mesh gets -1 and changes no bit of any other mesh; an index is judged against its OWN mesh's vertex count."""
    from genpc_amd.utils import mesh_io as M
    meshes = _bad_batch()
    seeds = [50 + j for j in range(7)]
    got = _ragged(meshes, 200, seeds)
    assert [g["status"] for g in got] == [1, -1, -1, -1, -1, 1, 1]
    for j in (0, 5, 6):
        V, F, C = meshes[j]
        _same(got[j], R.sample(V, F, 200, seeds[j], colors=C), "mesh %d" % j)
    for j in (1, 2, 3, 4):
        assert R.sample(meshes[j][0], meshes[j][1], 10, seeds[j])["status"] == -1, j
    assert (got[4]["face"] == -1).all() and (got[4]["points"] == 0).all() and (got[4]["colors"] == 0).all() and (got[4]["bary"] == 0).all()
    with pytest.raises(ValueError, match="mesh 1 cannot be sampled"):
        M.sample_surfaces_gpu(meshes, 200, seeds)
    # a following call is served
    ok = M.sample_surfaces_gpu([meshes[0], meshes[5]], 200, [seeds[0], seeds[5]], return_bary=True)
    for i, j in enumerate((0, 5)):
        for x, k in zip(ok[i], ("points", "face", "colors", "bary")):
            np.testing.assert_array_equal(x.cpu().numpy(), got[j][k])


def test_prefix_property_and_determinism():
    import torch
    from genpc_amd.utils import mesh_io as M
    dev = torch.device("cuda")
    a, b = R.grid_mesh(3000, seed=8), R.grid_mesh(700, seed=9)
    A, B = [tuple(torch.from_numpy(x).to(dev) for x in m) for m in (a, b)]
    # mesh A stands at positions 0 and 2 with the same seed
    long = M.sample_surfaces_gpu([A, B, A], [4097, 300, 4097], [21, 22, 21], return_bary=True)
    short = M.sample_surfaces_gpu([A, B, A], [100, 50, 257], [21, 22, 21], return_bary=True)
    assert len(long) == 3 and len(long[0]) == 4 and long[0][0].is_cuda and long[0][1].dtype == torch.int32
    for j, n in enumerate((100, 50, 257)):
        for x, y in zip(long[j], short[j]):
            assert y.shape[0] == n and torch.equal(x[:n], y), j
    for x, y in zip(long[0], long[2]):
        assert torch.equal(x, y)
    want = R.sample(a[0], a[1], 4097, 21, colors=a[2])
    for x, k in zip(long[2], ("points", "face", "colors", "bary")):
        np.testing.assert_array_equal(x.cpu().numpy(), want[k])
    again = M.sample_surfaces_gpu([A, B, A], [4097, 300, 4097], [21, 22, 21], return_bary=True)
    other = M.sample_surfaces_gpu([A, B, A], [4097, 300, 4097], [21, 23, 21], return_bary=True)
    # on a side stream beside another kernel in flight
    big = torch.randn(4096, 4096, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    prod = big @ big
    with torch.cuda.stream(side):
        beside = M.sample_surfaces_gpu([A, B, A], [4097, 300, 4097], [21, 22, 21], return_bary=True)
    side.synchronize()
    torch.cuda.synchronize()
    assert prod.shape == (4096, 4096)
    for j in range(3):
        for x, y, z in zip(long[j], again[j], beside[j]):
            assert torch.equal(x, y) and torch.equal(x, z), j
    assert torch.equal(long[0][0], other[0][0]) and not torch.equal(long[1][0], other[1][0])


def test_a_colourless_mesh_in_a_coloured_batch():
    """Constant 0.5 vertex colours interpolate to exactly 0.5: b0 + r1 + r2 = 1 exactly and every product and sum is exact."""
    from genpc_amd.utils import mesh_io as M
    m = [R.grid_mesh(nf, seed=30 + nf) for nf in (300, 1500, 40)]
    got = M.sample_surfaces_gpu([m[0], m[1][:2], m[2]], 4097, [5, 6, 7])
    assert all(len(t) == 3 for t in got)
    grey = got[1][2].cpu().numpy()
    assert grey.shape == (4097, 3) and grey.dtype == np.float32 and (grey == np.float32(0.5)).all()
    np.testing.assert_array_equal(got[1][0].cpu().numpy(), R.sample(m[1][0], m[1][1], 4097, 6)["points"])
    for j in (0, 2):
        want = R.sample(m[j][0], m[j][1], 4097, 5 + j, colors=m[j][2])
        np.testing.assert_array_equal(got[j][0].cpu().numpy(), want["points"])
        np.testing.assert_array_equal(got[j][2].cpu().numpy(), want["colors"])
    # no mesh brings colours: the tuples have none, as sample_surface_gpu's
    plain = M.sample_surfaces_gpu([m[0][:2], m[2][:2]], [10, 20], 3)
    assert [len(t) for t in plain] == [2, 2] and plain[1][0].shape == (20, 3)


def test_glb2points_gpu(tmp_path):
    import torch
    from genpc_amd.utils import mesh_io as M
    paths = []
    for j, (nu, nv) in enumerate(((48, 24), (32, 16), (20, 12))):
        verts, faces, cols = _ellipsoid_mesh(nu, nv)
        paths.append(str(tmp_path / ("m%d.glb" % j)))
        write_glb(paths[-1], verts, faces, None if j == 1 else cols, indices_u16=True)
    for down in (None, 0.05):
        got = M.glb2points_gpu(paths, down_sample=down, num_points=5000, seed=4)
        assert len(got) == 3
        for j, p in enumerate(paths):
            wp, wc = M.glb2point_gpu(p, down_sample=down, num_points=5000, seed=4)
            assert got[j][0].is_cuda and got[j][0].dtype == torch.float32 and got[j][0].shape == got[j][1].shape
            assert torch.equal(got[j][0], wp) and torch.equal(got[j][1], wc), (down, j)
            assert (down is None) == (got[j][0].shape[0] == 5000)
    assert bool((got[1][1] == 0.5).all())
    # one seed and one count per file
    per = M.glb2points_gpu(paths, num_points=[100, 200, 300], seed=[1, 2, 3])
    for j, p in enumerate(paths):
        wp, wc = M.glb2point_gpu(p, num_points=100 * (j + 1), seed=j + 1)
        assert torch.equal(per[j][0], wp) and torch.equal(per[j][1], wc)
    assert M.glb2points_gpu([]) == []
