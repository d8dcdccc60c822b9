"""Same input twice => identical output, for every entry point whose results the parity tests hold bit-exact
(SURVEY section 5's determinism checks) -- and a stated, tested bound for the one path that is
not run-to-run deterministic: the alignment loop (fp64 atomics in its reductions)."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def _twice(fn):
    a = fn()
    b = fn()
    a = a if isinstance(a, (tuple, list)) else (a,)
    b = b if isinstance(b, (tuple, list)) else (b,)
    return a, b


def _same(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert bool((x.view(-1).view(dtype=x.dtype) == y.view(-1)).all()) or (
            x.dtype.is_floating_point and bool(((x == y) | (x.isnan() & y.isnan())).all()))


def test_bit_exact_entry_points_repeat(env):
    torch = env
    from genpc_amd.loss_functions import chamfer_3DDist, emdModule
    from genpc_amd.fps import fps_sampling
    from genpc_amd import reg_xyz
    from genpc_amd.DepthPrompting import DepthPrompting
    from genpc_amd.ScaleAdapter import ScaleAdapter
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    A = torch.rand(2, 6000, 3, device="cuda", generator=g) - 0.5
    B = torch.rand(2, 5000, 3, device="cuda", generator=g) - 0.5
    _same(*_twice(lambda: chamfer_3DDist()(A, B)))
    X = torch.rand(2, 2048, 3, device="cuda", generator=g)
    Y = torch.rand(2, 2048, 3, device="cuda", generator=g)
    _same(*_twice(lambda: emdModule()(X, Y, 0.005, 50)))
    big = torch.rand(40000, 3, device="cuda", generator=g)
    _same(*_twice(lambda: fps_sampling(big, 3000)))
    col = torch.rand(40000, 3, device="cuda", generator=g)
    _same(*_twice(lambda: reg_xyz.voxel_down_sample(big, 0.03, colors=col)))
    _same(*_twice(lambda: reg_xyz.knn_mean_distance(big[:20000].contiguous(), 20)))
    cfg = SimpleNamespace(device="cuda", fovy=49.1, res=256, cam_res=256, padding=0.15, rescale=True, point_size=2,
                          mask_pixel_rate=3, view_num=32, distance=1.6, downsample_num=4000, removal_radius=10000)
    dp = DepthPrompting(cfg)
    pts = (big[:6000] - 0.5).contiguous()
    _same(*_twice(lambda: dp.getUvs(dp.cameras, pts)))
    _same(*_twice(lambda: dp.hidden_point_removal(pts, dp.viewpoints, 10000.0)[:2]))
    uv, depth, _ = dp.getUvs(dp.cameras[:1], pts)
    pix = dp.uvToPixels(uv[0], 256)
    _same(*_twice(lambda: dp.getRawDepth(pix, depth[0], colors=col[:6000].contiguous(), res=256, point_size=2, mask_pixel_rate=3)))
    img = torch.rand(3, 1024, 1024, device="cuda", generator=g)
    _same(*_twice(lambda: ScaleAdapter(cfg).colorPoint(uv[0], img)))
    # ICP / scale search: fp64 sums through atomics -> transforms agree to rounding, scores are bit-exact NN outputs
    S1, l1, T1 = reg_xyz.iterative_scale_search(pts[:3000].contiguous() * 0.9, pts[:4000].contiguous(), [(0.8, 1.2)] * 3, 6, cd_inv_weight=0.5)
    S2, l2, T2 = reg_xyz.iterative_scale_search(pts[:3000].contiguous() * 0.9, pts[:4000].contiguous(), [(0.8, 1.2)] * 3, 6, cd_inv_weight=0.5)
    assert l1 == l2 and np.array_equal(S1, S2)
    np.testing.assert_allclose(T1, T2, atol=1e-12)


def test_alignment_loop_repeats(env):
    """The alignment loop, same input twice: identical loss histories and transforms, Chamfer-only and full
    objective (white and coloured).  Its reductions are fp64 atomics over float-derived terms (their order varies,
    the float results do not: no difference seen in any run), and the splat fills its per-tile lists in ascending
    point order, so a pixel sums its discs in the same order every time.  (Round 2's arrival-order lists made the
    full objective drift run to run: 3e-5 after 5 steps, 3 % after 50 -- a last-bit difference in the image flips
    a soft-mask pixel in or out of fp32 sigmoid saturation and the loss jumps by 100 / P.)"""
    torch = env
    from genpc_amd.optim_registration.diff_obj_pose import object_pose_optimization
    rng = np.random.default_rng(5)
    u = rng.standard_normal((4000, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    complete = (u * np.array([0.5, 0.3, 0.2])).astype(np.float32)
    complete[:600] += np.float32([0.15, 0.1, 0.0]) * np.abs(u[:600, :1]).astype(np.float32)
    th = math.radians(10.0)
    Rt = np.array([[math.cos(th), 0, math.sin(th)], [0, 1, 0], [-math.sin(th), 0, math.cos(th)]])
    c = complete.mean(0)
    full = ((complete - c) * 0.9) @ Rt.T + c + np.array([0.02, -0.01, 0.015])
    partial = full[full[:, 2] > -0.05][:2000].astype(np.float32)
    C, P = torch.from_numpy(complete).cuda(), torch.from_numpy(partial).cuda()
    col = torch.from_numpy((0.2 + 0.8 * rng.random((4000, 3))).astype(np.float32)).cuda()
    pcol = torch.from_numpy((0.2 + 0.8 * rng.random((len(partial), 3))).astype(np.float32)).cuda()
    for kw in (dict(cd_only=True), dict(radius=0.02), dict(radius=0.02, complete_col=col, partial_col=pcol)):
        runs = [object_pose_optimization(C, P, lr=0.01, iters=60, return_history=True, **kw) for _ in range(3)]
        for T, h, bp in runs[1:]:
            np.testing.assert_array_equal(h, runs[0][1], err_msg=str(list(kw)))
            np.testing.assert_array_equal(T, runs[0][0], err_msg=str(list(kw)))


def test_seeded_nearest_neighbours_give_the_brute_force_histories(golden):
    """The alignment loop answers its nearest-neighbour queries from the second step on by a seeded cell search
    (csrc/nn_seeded.hip: last step's index bounds the ball to search; the moving cloud's grid lives in its rest frame);
    switched off (genpc_pose_tune(0)) every step runs the brute-force filter.  Transforms, the loss history of every
    start and the winning parameters are IDENTICAL -- on a bundled scan against its ground truth (half of the complete
    cloud has no near partial point), on the Waymo pair with its pad-repeated crop (exact duplicates: index ties), on a
    coloured lock-step batch, and with the silhouette term off."""
    import torch
    from genpc_amd import _lib
    from genpc_amd.optim_registration.diff_obj_pose import object_pose_optimization
    L = _lib.lib
    g = golden("scans13_fps16384.npz")
    w = golden("waymo_car59_4096.npz")
    rng = np.random.default_rng(2)
    cases = [("scan", g["gt"][3][:8192].copy(), g["partial"][3][:4096].copy(), {}),
             ("waymo_pair", w["complete"], w["test_partial"], {}),
             ("cd_only", g["gt"][5][:6000].copy(), g["partial"][5][:3000].copy(), {"cd_only": True}),
             ("batch3", np.stack([g["gt"][k][:5000] for k in (0, 1, 2)]), np.stack([g["partial"][k][:2500] for k in (0, 1, 2)]), {})]
    for name, C, P, kw in cases:
        c = (C - C.mean(-2, keepdims=True)) / np.ptp(C.reshape(-1, 3), axis=0).max()
        p = (P - C.mean(-2, keepdims=True)) / np.ptp(C.reshape(-1, 3), axis=0).max() * 0.85 + 0.01
        Ct, Pt = torch.from_numpy(c.astype(np.float32)).cuda(), torch.from_numpy(p.astype(np.float32)).cuda()
        out = []
        for seeded in (1, 0):
            prev = L.genpc_pose_tune(seeded)
            try:
                out.append(object_pose_optimization(Ct, Pt, radius=0.02, lr=0.01, iters=60, render_size=224, return_history=True, **kw))
            finally:
                L.genpc_pose_tune(prev)
        for a, b_ in zip(out[0], out[1]):
            np.testing.assert_array_equal(np.asarray(a), np.asarray(b_), err_msg=name)


def test_adaptive_nearest_neighbours_give_the_brute_force_histories(env):
    """Mode 2 (genpc_pose_tune(2), the default where the clouds are large): the loop times the filter at steps 0 and 2, a
    SAMPLED seeded launch in front of the filter at step 1, and from then on probes again every so often and runs whichever
    was faster -- 30 steps reach the second probe (step 26), which may be a full seeded search.  Whatever the timings choose,
    transforms, the loss history of every start and the winning parameters are IDENTICAL to the brute-force filter's
    (genpc_pose_tune(0)), with the silhouette term and without it.  Small synthetic clouds: 1024 points on an ellipsoid
    against 512 of its posed front half (a thread that asks for a mode gets it at any size from 256 points)."""
    torch = env
    from genpc_amd import _lib
    from genpc_amd.optim_registration.diff_obj_pose import object_pose_optimization
    L = _lib.lib
    rng = np.random.default_rng(17)
    u = rng.standard_normal((1024, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    complete = (u * np.array([0.5, 0.3, 0.2])).astype(np.float32)
    th = math.radians(11.0)
    Rt = np.array([[math.cos(th), 0, math.sin(th)], [0, 1, 0], [-math.sin(th), 0, math.cos(th)]])
    c = complete.mean(0)
    full = ((complete - c) * 0.9) @ Rt.T + c + np.array([0.02, -0.01, 0.015])
    front = full[full[:, 2] > np.median(full[:, 2])]
    assert len(front) == 512
    partial = front.astype(np.float32)
    C, P = torch.from_numpy(complete).cuda(), torch.from_numpy(partial).cuda()
    for kw in (dict(radius=0.02, render_size=224), dict(cd_only=True)):
        out = []
        for mode in (2, 0):
            prev = L.genpc_pose_tune(mode)
            try:
                out.append(object_pose_optimization(C, P, lr=0.01, iters=30, return_history=True, **kw))
            finally:
                L.genpc_pose_tune(prev)
        assert np.asarray(out[0][1]).shape == (4, 31) and np.isfinite(np.asarray(out[0][1])).all()
        for a, b_ in zip(out[0], out[1]):
            np.testing.assert_array_equal(np.asarray(a), np.asarray(b_), err_msg=str(list(kw)))
