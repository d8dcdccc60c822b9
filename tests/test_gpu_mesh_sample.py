"""The device mesh sampler (csrc/mesh_sample.hip -> genpc_mesh_sample -> utils/mesh_io.sample_surface_gpu) against the numpy
restatement of its definition (tests/mesh_sample_ref.py).  Every comparison is bit for bit: points, faces, barycentric
weights, colours and the integer face weights the library leaves in its workspace -- the latter is what measures that the
fp64 square root of this part is correctly rounded, as numpy's is."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import mesh_sample_ref as R
from conftest import write_glb

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 4097)          # partial waves, a partial last workgroup


def _run(V, F, count, seed, C=None):
    """One library call -> numpy dict (points, face, bary, colors, status, w, cum)."""
    from genpc_amd.utils import mesh_io as M
    r = M._mesh_sample(V, F, count, seed, colors=C, want_bary=True)
    w, cum = M.mesh_sample_weights(r["workspace"], r["nf"])
    return dict(points=r["points"].cpu().numpy(), face=r["face"].cpu().numpy(), bary=r["bary"].cpu().numpy(),
                colors=None if r["colors"] is None else r["colors"].cpu().numpy(), status=int(r["status"].item()), w=w, cum=cum)


def _same(got, want, n=None):
    assert got["status"] == want["status"] == 1
    for k in ("points", "face", "bary", "colors"):
        if want[k] is None:
            assert got[k] is None
        else:
            assert got[k].dtype == want[k].dtype, k
            np.testing.assert_array_equal(got[k], want[k][:n], err_msg=k)


@pytest.mark.parametrize("nf", [1, 2, 255, 256, 257, 1024, 1025, 5000])
def test_sizes_bit_for_bit(nf):
    """One face, the workgroup-scan boundaries (a lane holds 4 faces, a wave 256, a workgroup 1024) and the second search
    level (more than one chunk of 1024 faces), at every count."""
    V, F, C = R.grid_mesh(nf, seed=nf)
    want = R.sample(V, F, max(COUNTS), seed=1000 + nf, colors=C)
    for count in COUNTS:
        got = _run(V, F, count, 1000 + nf, C)
        np.testing.assert_array_equal(got["w"], want["w"])
        np.testing.assert_array_equal(got["cum"], want["cum"])
        _same(got, want, count)
    assert len(np.unique(want["face"])) > min(nf, 4097) // 4          # (the comparison is not of a constant)


@pytest.mark.parametrize("scale", [1.0, 2.0 ** -60, 3e-7, 7e9])
def test_weights_measure_the_fp64_root(scale):
    """20 000 random triangles at four scales: 20 000 fp64 roots a case, each compared through floor(A * 2^k) with
    numpy's correctly rounded root (a root one ulp off moves a weight that has all 39 bits of the largest face's, and
    the bits below in the smaller ones, so most wrong roots show; every weight must be equal)."""
    rng = np.random.default_rng(17)
    V = (rng.standard_normal((30000, 3)) * scale).astype(np.float32)
    F = rng.integers(0, len(V), (20000, 3)).astype(np.int32)
    got = _run(V, F, 64, 3)
    w, cum, bad = R.face_weights(V, F)
    assert not bad and got["status"] == 1
    np.testing.assert_array_equal(got["w"], w)
    np.testing.assert_array_equal(got["cum"], cum)
    assert int(w.max()) >= 1 << 38
    _same(got, R.sample(V, F, 64, 3))


def test_zero_weight_faces_are_never_drawn():
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0],
                  [2, 0, 0], [2, 1, 0],
                  [3, 0, 0], [4, 0, 0], [3, 1, 0],
                  [5, 0, 0], [5 + 2.0 ** -20, 0, 0], [5, 2.0 ** -20, 0]], np.float32)
    F = np.array([[0, 1, 2], [3, 3, 4], [5, 6, 7], [8, 9, 10]], np.int32)       # 1: degenerate; 3: 2^-40 of face 0's area
    got = _run(V, F, 50000, 5)
    assert got["w"][1] == 0 and got["w"][3] == 0
    assert set(np.unique(got["face"])) == {0, 2}
    _same(got, R.sample(V, F, 50000, 5))
    # every face degenerate: status -1, and the Python call says why
    from genpc_amd.utils import mesh_io as M
    G = np.array([[3, 3, 4], [0, 0, 0]], np.int32)
    assert _run(V, G, 100, 5)["status"] == -1
    with pytest.raises(ValueError, match="all face weights zero"):
        M.sample_surface_gpu(V, G, 100, 5)


def test_prefix_property():
    V, F, C = R.grid_mesh(3000, seed=8)
    a, b = _run(V, F, 4097, 21, C), _run(V, F, 100, 21, C)
    for k in ("points", "face", "bary", "colors"):
        np.testing.assert_array_equal(a[k][:100], b[k], err_msg=k)


def test_determinism_seeds_and_side_stream():
    import torch
    from genpc_amd.utils import mesh_io as M
    V, F, C = R.grid_mesh(2500, seed=9)
    dev = torch.device("cuda")
    Vd, Fd, Cd = torch.from_numpy(V).to(dev), torch.from_numpy(F).to(dev), torch.from_numpy(C).to(dev)
    a = M.sample_surface_gpu(Vd, Fd, 4097, 33, colors=Cd, return_bary=True)
    b = M.sample_surface_gpu(Vd, Fd, 4097, 33, colors=Cd, return_bary=True)
    c = M.sample_surface_gpu(Vd, Fd, 4097, 34, colors=Cd, return_bary=True)
    assert len(a) == 4 and a[0].is_cuda and a[0].dtype == torch.float32 and a[1].dtype == torch.int32
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    # on a side stream beside another kernel in flight
    big = torch.randn(4096, 4096, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    prod = big @ big
    with torch.cuda.stream(side):
        d = M.sample_surface_gpu(Vd, Fd, 4097, 33, colors=Cd, return_bary=True)
    side.synchronize()
    torch.cuda.synchronize()
    assert prod.shape == (4096, 4096)
    for x, y in zip(a, d):
        assert torch.equal(x, y)
    want = R.sample(V, F, 4097, 33, colors=C)
    np.testing.assert_array_equal(a[0].cpu().numpy(), want["points"])


@pytest.mark.parametrize("case", ["index_nv", "index_minus_1", "nan_vertex"])
def test_bad_faces_give_status_minus_1(case):
    """The kernel checks an index before it loads through it; a bad mesh raises and the next call is served."""
    from genpc_amd.utils import mesh_io as M
    V, F, C = R.grid_mesh(600, seed=10)
    G = F.copy()
    if case == "index_nv":
        G[300, 1] = len(V)
    elif case == "index_minus_1":
        G[599, 2] = -1
    else:
        V = V.copy()
        V[int(F[17, 0]), 1] = np.nan
    assert R.sample(V, G, 10, 1)["status"] == -1
    assert _run(V, G, 200, 1, C)["status"] == -1
    with pytest.raises(ValueError, match="outside"):
        M.sample_surface_gpu(V, G, 200, 1, colors=C)
    # a NaN vertex that no face uses is fine, and the process is healthy
    U = np.concatenate([R.grid_mesh(600, seed=10)[0], np.full((1, 3), np.nan, np.float32)])
    _same(_run(U, F, 200, 1), R.sample(U, F, 200, 1))


def test_colours_and_the_clamp():
    V, F, _ = R.grid_mesh(300, seed=11)
    rng = np.random.default_rng(12)
    C = rng.choice(np.array([0.0, 1.0, 1.5, -0.25, 0.3], np.float32), size=V.shape).astype(np.float32)
    want = R.sample(V, F, 4097, 6, colors=C)
    got = _run(V, F, 4097, 6, C)
    _same(got, want)
    assert (got["colors"] == 0).any() and (got["colors"] == 1).any() and got["colors"].min() >= 0 and got["colors"].max() <= 1
    raw = (C.astype(np.float64)[F[want["face"]]] * want["bary"].astype(np.float64)[:, :, None]).sum(1)
    assert (raw > 1).any() and (raw < 0).any()                        # the clamp had work to do


def test_host_refusals():
    import torch
    from genpc_amd import _lib
    from genpc_amd.utils import mesh_io as M
    L, p = _lib.lib, _lib.ptr
    dev = torch.device("cuda")
    V, F, C = [torch.from_numpy(a).to(dev) for a in R.grid_mesh(10, seed=1)]
    ws = torch.empty(L.genpc_mesh_sample_bytes(10), dtype=torch.uint8, device=dev)
    out, outc = torch.empty(8, 3, device=dev), torch.empty(8, 3, device=dev)
    st = torch.full((1,), 7, dtype=torch.int32, device=dev)

    def call(nv=len(V), nf=10, count=8, colors=None, out_colors=None):
        return _lib.on_device_of(V, L.genpc_mesh_sample, nv, p(V), p(colors), nf, p(F), count, 1, p(out), p(out_colors), p(None),
                                 p(None), p(st), p(ws))
    assert call(out_colors=outc) == -1 and "out_colors without vertex_colors" in _lib.last_error()
    assert call(nf=0) == -1 and call(nf=(1 << 24) + 1) == -1 and call(count=0) == -1 and call(nv=0) == -1
    assert L.genpc_mesh_sample_bytes(0) == -1 and L.genpc_mesh_sample_bytes((1 << 24) + 1) == -1
    assert 0 < L.genpc_mesh_sample_bytes(1 << 24) < 1 << 31
    torch.cuda.synchronize()
    assert int(st.item()) == 7                                        # nothing was enqueued
    assert call(colors=C, out_colors=outc) == 1 and int(st.item()) == 1
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        M.sample_surface_gpu(V.cpu(), F, 8, 0)
    with pytest.raises(TypeError):
        M.sample_surface_gpu(V, F, 8, 0.5)
    with pytest.raises(ValueError):
        M.sample_surface_gpu(V, F, 0, 0)


def _ellipsoid_mesh(nu=48, nv=24, radii=(0.45, 0.3, 0.2)):
    u = np.linspace(0, 2 * np.pi, nu, endpoint=False)
    v = np.linspace(0.05, np.pi - 0.05, nv)
    uu, vv = np.meshgrid(u, v)
    verts = np.stack([radii[0] * np.cos(uu) * np.sin(vv), radii[1] * np.cos(vv), radii[2] * np.sin(uu) * np.sin(vv)], -1).reshape(-1, 3)
    verts[:, 0] += 0.12 * (verts[:, 1] > 0.1)            # a bump: no symmetry for the pose to slide on
    faces = []
    for j in range(nv - 1):
        for i in range(nu):
            a, b = j * nu + i, j * nu + (i + 1) % nu
            faces += [[a, b, a + nu], [b, b + nu, a + nu]]
    cols = 0.2 + 0.8 * (verts - verts.min(0)) / (verts.max(0) - verts.min(0))
    return verts, np.array(faces), cols


def test_glb2point_gpu(tmp_path):
    import torch
    from genpc_amd.utils import dataUtils as D, mesh_io as M
    verts, faces, cols = _ellipsoid_mesh()
    glb = str(tmp_path / "m.glb")
    write_glb(glb, verts, faces, cols, indices_u16=True)
    V, F, C = M.load_glb(glb)
    pts, col = M.glb2point_gpu(glb, num_points=5000, seed=4)
    assert pts.is_cuda and col.is_cuda and pts.shape == col.shape == (5000, 3) and pts.dtype == col.dtype == torch.float32
    want = M.sample_surface_gpu(V, F, 5000, 4, colors=C)
    assert torch.equal(pts, want[0]) and torch.equal(col, want[2])
    ref = R.sample(V, F, 5000, 4, colors=C)
    np.testing.assert_array_equal(pts.cpu().numpy(), ref["points"])
    np.testing.assert_array_equal(col.cpu().numpy(), ref["colors"])
    # with down_sample: the library's voxel grid over those samples
    dp, dc = M.glb2point_gpu(glb, down_sample=0.05, num_points=5000, seed=4)
    wp, wc = D.voxel_down_sample_colored(pts.cpu().numpy(), col.cpu().numpy(), 0.05)
    assert dp.is_cuda and 0 < len(dp) < 5000
    np.testing.assert_array_equal(dp.cpu().numpy(), wp)
    np.testing.assert_array_equal(dc.cpu().numpy(), wc)
    # a file without colours: 0.5 grey
    write_glb(glb, verts, faces, None, indices_u16=True)
    gp, gc = M.glb2point_gpu(glb, num_points=100, seed=4)
    assert torch.equal(gp, pts[:100]) and bool((gc == 0.5).all())


def test_reg_with_a_seed_is_reproducible(tmp_path):
    """reg(cfg, flag, seed=7) on a tiny stage-2 directory: both mesh samplings come from the device sampler, and two runs
    write byte-identical fused clouds."""
    import torch
    from genpc_amd import reg_xyz
    from genpc_amd.utils import dataUtils as D, mesh_io as M
    flag = "00042"
    base = tmp_path / flag
    os.makedirs(base)
    cfg = SimpleNamespace(output_path=str(tmp_path), device="cuda", generative_model="trellis", dataset="redwood")
    verts, faces, cols = _ellipsoid_mesh()
    glb = str(base / (flag + "_trellis.glb"))
    write_glb(glb, verts, faces, cols, indices_u16=True)
    # the observed partial cloud: the mesh's front half, at 0.88 scale and slightly moved, with the mesh's colours
    pts, pcols = M.glb2point_gpu(glb, num_points=6000, seed=5)
    pts, pcols = pts.cpu().numpy(), pcols.cpu().numpy()
    front = pts[:, 2] > -0.02
    partial = (pts[front] * 0.88 + np.array([0.015, -0.01, 0.01])).astype(np.float32)
    D.save_ply_xyzrgb(partial, pcols[front], str(base / "color_point.ply"))
    with pytest.raises(TypeError, match="exclude"):
        reg_xyz.reg(cfg, flag, seed=7, rng=np.random.default_rng(0))
    with pytest.raises(TypeError, match="unexpected keyword"):
        reg_xyz.reg(cfg, flag, seed=7, sead=7)
    with pytest.raises(TypeError):
        reg_xyz.reg(cfg, flag, seed="7")
    fused_path = str(base / (flag + "_fused.ply"))
    cwd = os.getcwd()
    os.chdir(str(tmp_path))              # the pose initialisation drops its side-effect files into the working directory
    try:
        blobs = []
        for _ in range(2):
            out = reg_xyz.reg(cfg, flag, seed=7)
            assert out["fused_path"] == fused_path
            with open(fused_path, "rb") as f:
                blobs.append(f.read())
            os.remove(fused_path)
    finally:
        os.chdir(cwd)
    assert blobs[0] == blobs[1] and len(blobs[0]) > 10000 * 27
    # the complete cloud reg() aligned is the seeded sampling of the mesh, moved rigidly and scaled: same point count
    assert out["target"].shape == (163840, 3) and out["target_col"].shape == (163840, 3)
    want = M.glb2point_gpu(glb, num_points=163840, seed=7)[1]
    assert torch.equal(out["target_col"], want)


def test_mesh_cd_emd():
    from genpc_amd import metric
    verts, faces, _ = _ellipsoid_mesh()
    kw = dict(samples=8192, points=2048)
    cd_same, emd_same = metric.mesh_cd_emd(verts, faces, verts, faces, seed=3, **kw)
    assert float(cd_same) == 0.0 and float(emd_same) >= 0.0
    cd_two, emd_two = metric.mesh_cd_emd(verts, faces, verts, faces, seed=(3, 4), **kw)
    assert 0.0 < float(cd_two) < 0.05 and 0.0 < float(emd_two) < 0.1
    cd_big, _ = metric.mesh_cd_emd(verts, faces, verts * 1.1, faces, seed=(3, 4), **kw)
    assert float(cd_big) > float(cd_two)
