"""Parity of the projection / splat / colour-gather / pose kernels against the CPU
oracle (oracle/genpc_oracle_geom.c).  Bar: projection, pixels, splat and gather
BIT-EXACT (no reduction order is involved: min/max are exact); pose transform 2
ulp (device expf vs libm expf); pose gradient 1e-4 relative (fp64 reductions in a
different order); the optimisation loop by outcome (same basin, transform within
1e-2, loss history within 2 %)."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import gen_pair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gp():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import DepthPrompting as DP
    from genpc_amd.ScaleAdapter import ScaleAdapter
    from genpc_amd.optim_registration import diff_obj_pose as POSE
    cfg = SimpleNamespace(device="cuda", fovy=49.1, res=256, padding=0.15, rescale=True, point_size=1,
                          mask_pixel_rate=3, view_num=16, distance=1.6)
    return dict(torch=torch, DP=DP, dp=DP.DepthPrompting(cfg), sa=ScaleAdapter(cfg), POSE=POSE, cfg=cfg)


def test_cameras_match_oracle(gp, oracle):
    views, eyes, focal = gp["DP"].create_cameras(16, 1.6, 49.1, "cuda")
    oe = oracle.fibonacci_sphere(16, 1.6)
    np.testing.assert_array_equal(eyes, oe)
    ov = np.stack([oracle.look_at(e, np.zeros(3), oracle.calculate_up_vector(e, np.zeros(3))) for e in oe])
    np.testing.assert_allclose(views.cpu().numpy(), ov, atol=2e-7)


@pytest.mark.parametrize("n,c,rescale", [(1, 1, True), (5000, 16, True), (71372, 2, True), (3000, 4, False)])
def test_get_uvs_bit_exact(gp, oracle, n, c, rescale):
    torch = gp["torch"]
    a, _ = gen_pair(n, (1, n, 3), (1, 1, 3))
    xyz = a[0] * 0.8
    views = gp["dp"].cameras[:c]
    uv, depth, tr = gp["dp"].getUvs(views, torch.from_numpy(xyz).cuda(), rescale=rescale, padding=0.15)
    ouv, od, otr, _ = oracle.get_uvs(views.cpu().numpy(), gp["dp"].focal, xyz, rescale=rescale, padding=0.15)
    if n == 1 and rescale:      # degenerate bbox: 0/0 in the reference too
        assert np.isnan(uv.cpu().numpy()).all() and np.isnan(ouv).all()
    else:
        np.testing.assert_array_equal(uv.cpu().numpy(), ouv)
    np.testing.assert_array_equal(depth.cpu().numpy(), od)
    np.testing.assert_array_equal(tr.cpu().numpy(), otr)


@pytest.mark.parametrize("point_size", [1, 2, 3])
def test_paint_pixels_and_raw_depth(gp, oracle, point_size):
    torch = gp["torch"]
    rng = np.random.default_rng(point_size)
    n, res = 4000, 256
    uv = rng.random((n, 2), dtype=np.float32) * 1.1 - 0.05          # some out of range -> clipped
    pix = gp["dp"].uvToPixels(torch.from_numpy(uv).cuda(), res)
    opix = oracle.uv_to_pixels(uv, res)
    np.testing.assert_array_equal(pix.cpu().numpy(), opix)
    col = rng.random((n, 3), dtype=np.float32)
    img = torch.zeros(3, res, res, device="cuda")
    out = gp["dp"].paintPixels(img, pix, torch.from_numpy(col).cuda(), point_size)
    oout, oimg = oracle.paint_pixels(res, opix, col, point_size)
    np.testing.assert_array_equal(out.cpu().numpy(), oout)
    np.testing.assert_array_equal(img.cpu().numpy(), oimg)
    # getRawDepth end to end against the same composition on the oracle
    depth = rng.random(n, dtype=np.float32)
    gp["cfg"].point_size = point_size
    s_img, s_depth, h1, h2 = gp["dp"].getRawDepth(pix, torch.from_numpy(depth).cuda(), colors=torch.from_numpy(col).cuda(),
                                                  res=res, point_size=point_size, mask_pixel_rate=3)
    grey = (np.float32(0.1) + np.float32(0.8) * (1 - (depth - depth.min()) / (depth.max() - depth.min()))).astype(np.float32)
    o_depth, _ = oracle.paint_pixels(res, opix, np.repeat(grey[:, None], 3, 1), point_size)
    np.testing.assert_allclose(s_depth.cpu().numpy(), o_depth, atol=1e-7)
    np.testing.assert_array_equal(s_img.cpu().numpy(), oout)
    o_all, _ = oracle.paint_pixels(res, opix, col, point_size * 3)
    front_all, front = (o_all != 0), (oout != 0)
    np.testing.assert_array_equal(h1.cpu().numpy() != 0, front_all ^ front)       # all_back ^ back == all_front ^ front
    np.testing.assert_array_equal(h2.cpu().numpy() != 0, front_all ^ ~front)


def test_color_point_gather(gp, oracle):
    torch = gp["torch"]
    rng = np.random.default_rng(4)
    n = 8192
    uv = rng.random((n, 2), dtype=np.float32)
    img = rng.random((3, 1024, 1024), dtype=np.float32)
    got = gp["sa"].colorPoint(torch.from_numpy(uv).cuda(), torch.from_numpy(img).cuda())
    exp = oracle.gather_colors(oracle.uv_to_pixels(uv, 1024), img)
    np.testing.assert_array_equal(got.cpu().numpy(), exp)
    with pytest.raises(ValueError):
        gp["sa"].colorPoint(torch.from_numpy(uv).cuda(), torch.zeros(3, 512, 512).cuda())


def _shape(seed, n=4000):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    complete = (u * np.array([0.5, 0.3, 0.2])).astype(np.float32)
    k = n // 6
    complete[:k] += np.float32([0.15, 0.1, 0.0]) * np.abs(u[:k, :1]).astype(np.float32)
    th = math.radians(12.0)
    Rt = np.array([[math.cos(th), 0, math.sin(th)], [0, 1, 0], [-math.sin(th), 0, math.cos(th)]])
    c = complete.mean(0)
    full = ((complete - c) * 0.9) @ Rt.T + c + np.array([0.02, -0.01, 0.015])
    partial = full[full[:, 2] > -0.05][: n // 2].astype(np.float32)
    return complete, partial, Rt


def test_pose_transform_and_gradient(gp, oracle):
    torch = gp["torch"]
    complete, partial, _ = _shape(3, 3000)
    params = np.array([0.9, 0.1, -0.3, 0.05, 1.1, 0.2, 0.02, -0.01, 0.03, math.log(0.8)], np.float32)
    c = complete.astype(np.float64).mean(0).astype(np.float32)
    C, P, PR, CT = (torch.from_numpy(x).cuda() for x in (complete, partial, params, c))
    pts = gp["POSE"].pose_transform(C, CT, PR)
    opts = oracle.pose_transform(complete, c, params)
    np.testing.assert_allclose(pts.cpu().numpy(), opts, rtol=3e-7, atol=2e-7)
    loss, grad = gp["POSE"].pose_cd_loss_grad(C, CT, PR, P)
    d1, d2, i1, i2 = oracle.chamfer_forward(opts[None], partial[None], 1)
    lo, g = oracle.pose_loss_grad(complete, c, params, partial, d1[0], i1[0], d2[0], i2[0])
    np.testing.assert_allclose(loss.cpu().numpy(), lo, rtol=2e-5, atol=1e-6)
    # The gradient is a sum of ~4500 signed per-point terms; the kernel forms them from the fp32
    # posed points and fp32 reference distances (as torch's fp32 autograd would), the oracle from the
    # same inputs: agreement is 1e-4 of the gradient's magnitude per parameter group (rotation,
    # translation, scale), which is what cancellation in fp32 inputs allows.
    gg, go = grad.cpu().numpy().astype(np.float64), g.astype(np.float64)
    for sl in (slice(0, 6), slice(6, 9), slice(9, 10)):
        assert np.abs(gg[sl] - go[sl]).max() <= 1e-4 * np.abs(go[sl]).max(), (sl, gg[sl], go[sl])


def _colours(rng, n, dark=0.0):
    col = (0.25 + 0.75 * rng.random((n, 3))).astype(np.float32)
    k = int(n * dark)
    if k:
        col[:k] *= np.float32(0.08)
    return col


@pytest.fixture(autouse=True, params=[1, 0], ids=["pulsar_blend", "coverage_splat"])
def render_blend(request, gp, oracle):
    """Every test of this file runs with both renderers of the mask term, the library and the oracle switched together:
    Pulsar's published blending function (softmax in depth; the default since round 5) and the coverage splat."""
    from genpc_amd import _lib
    prev_l = _lib.lib.genpc_render_tune(request.param)
    prev_o = oracle.set_blend(request.param)
    yield request.param
    _lib.lib.genpc_render_tune(prev_l)
    oracle.set_blend(prev_o)


def _close_images(img, ref, blend):
    """fp32 (u, v, rho) against the oracle's fp64: 2e-4 for the coverage splat, whose image fades to 0 at a disc's rim.
    Pulsar's blending function has a HARD rim (any coverage > 0 outweighs the background by e^40), so a rim pixel whose
    coverage is positive in one precision and not in the other differs by the disc's whole colour: at most a few pixels in
    100 000 may, every other pixel within 1e-3 (the softmax weights are ratios of exponentials of fp32 depths)."""
    if blend == 0:
        np.testing.assert_allclose(img, ref, atol=2e-4)
        return
    bad = np.abs(img.astype(np.float64) - ref).max(-1) > 1e-3
    assert bad.sum() <= max(3, bad.size // 20000), (int(bad.sum()), bad.size)


def test_pulsar_blend_hides_the_back_surface(gp, oracle, render_blend):
    """What distinguishes the two renderers: two coincident discs, red in front of green."""
    torch = gp["torch"]
    two = torch.tensor([[0.0, 0.0, 0.3], [0.0, 0.0, -0.3]]).cuda()
    tc = torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]).cuda()
    px = gp["POSE"].splat_image(two, 0.05, 64, tc)[32, 32].cpu().numpy()
    if render_blend == 1:
        assert px[0] > 0.99 and px[1] < 1e-4
    else:
        assert 0.2 < px[0] < 0.8 and 0.2 < px[1] < 0.8


def test_splat_image_vs_oracle(gp, oracle, render_blend):
    """The colour splat (the build's stand-in for the reference's Pulsar renders): [S,S,3] image of a
    cloud against the oracle's fp64 restatement, several radii and image sizes, white and coloured."""
    torch = gp["torch"]
    complete, partial, _ = _shape(5, 4000)
    col = _colours(np.random.default_rng(1), len(partial), 0.3)
    for radius, size in ((0.02, 224), (0.022, 224), (0.05, 96), (0.005, 224), (0.02, 57)):
        for c in (None, col):
            img = gp["POSE"].splat_image(torch.from_numpy(partial).cuda(), radius, size,
                                         None if c is None else torch.from_numpy(c).cuda()).cpu().numpy()
            ref = oracle.splat_image(partial, radius, size, c)
            assert img.shape == (size, size, 3)
            _close_images(img, ref, render_blend)
            assert 0.002 < img.mean() < 0.9
            if c is None:
                assert np.array_equal(img[..., 0], img[..., 1]) and np.array_equal(img[..., 0], img[..., 2])
    # a cloud the camera does not see, and an empty one
    far = torch.tensor([[0.0, 0.0, 4.0], [0.0, 0.0, -2.5]]).cuda()
    assert float(gp["POSE"].splat_image(far, 0.05, 32).abs().max()) == 0.0
    assert float(gp["POSE"].splat_image(torch.zeros(0, 3).cuda(), 0.05, 32).abs().max()) == 0.0


def test_splat_tile_lists_and_their_fallbacks(gp, oracle, render_blend):
    """The splat reads per-tile index lists the projection kernel fills (mask.h bin_points_block).  The cases a list
    cannot hold must give the same image through the full scan: a tile hit by more points than a list holds (and one whose
    list is longer than one fill of the splat's LDS list), discs
    over more tiles than a point may be listed in, an image with more tiles than the block histogram, and a mixture
    (a dense knot inside an ordinary cloud: crowded and ordinary tiles in one image)."""
    torch = gp["torch"]
    rng = np.random.default_rng(77)
    _, partial, _ = _shape(6, 3000)
    knot = (partial[:1] + 0.004 * rng.standard_normal((9000, 3))).astype(np.float32)      # more than a list holds (8192)
    cases = (
        ("crowded tile", knot, 0.01, 224),
        ("crowded tile, a list of three fills", np.concatenate([partial, knot[:2500]]), 0.01, 224),
        ("knot in a cloud", np.concatenate([partial, knot]), 0.02, 224),
        ("wide discs", partial[:600], 0.3, 224),
        ("wide and narrow", np.concatenate([partial[:2000], partial[:1]]), 0.09, 160),
        ("large image", partial, 0.02, 640),
        ("one tile", partial[:500], 0.05, 16),
        ("long lists (bitmap ranks)", _shape(8, 12000)[0], 0.008, 96),
    )
    for name, pts, radius, size in cases:
        col = _colours(rng, len(pts), 0.2)
        for c in (None, col):
            img = gp["POSE"].splat_image(torch.from_numpy(pts).cuda(), radius, size,
                                         None if c is None else torch.from_numpy(c).cuda()).cpu().numpy()
            ref = oracle.splat_image(pts, radius, size, c)
            _close_images(img, ref, render_blend)
        # twice through the same scratch: the splat hands the counters back zeroed
        again = gp["POSE"].splat_image(torch.from_numpy(pts).cuda(), radius, size, torch.from_numpy(col).cuda()).cpu().numpy()
        np.testing.assert_allclose(again, img, atol=1e-6, err_msg=name)


def test_splat_fuzz(gp, oracle, render_blend):
    """Random clouds, sizes, radii and image sizes through the splat's tile lists (empty tiles, one-entry lists, lists
    ranked by counting and by bitmap, several fills, overflow, images with no lists) against the oracle's image."""
    torch = gp["torch"]
    rng = np.random.default_rng(2024)
    for case in range(16):
        n = int(rng.choice([1, 2, 63, 300, 2000, 9000, 20000]))
        size = int(rng.choice([16, 31, 57, 96, 224, 300, 528]))
        radius = float(rng.choice([0.004, 0.01, 0.02, 0.05, 0.11]))
        spread = float(rng.choice([0.02, 0.15, 0.45]))
        pts = (rng.standard_normal((n, 3)) * spread * np.array([1.0, 0.8, 0.5]) + rng.uniform(-0.2, 0.2, 3)).astype(np.float32)
        col = _colours(rng, n, 0.2) if case % 2 else None
        img = gp["POSE"].splat_image(torch.from_numpy(pts).cuda(), radius, size,
                                     None if col is None else torch.from_numpy(col).cuda()).cpu().numpy()
        ref = oracle.splat_image(pts, radius, size, col)
        _close_images(img, ref, render_blend)


def test_mask_gradient_on_crowded_wide_and_listless_images(gp, oracle):
    """The loss and gradient of the mask term where the splat's tile lists are at their limits: a tile whose list overflowed
    (drawn by the full scan), a long list, discs over more than four tiles (in no list), tiles of both widths, an image of
    more than 1024 tiles (no lists), a single tile.  Each against the oracle's full loss and gradient, and again through the
    same scratch (the lists are handed back empty)."""
    torch = gp["torch"]
    rng = np.random.default_rng(5)
    complete, partial, _ = _shape(4, 2500)
    knot = (complete[:1] + 0.004 * rng.standard_normal((9000, 3))).astype(np.float32)      # more than a list holds (8192)
    params = np.array([0.95, 0.05, -0.2, 0.02, 1.05, 0.1, 0.01, -0.02, 0.02, math.log(0.85)], np.float32)
    cases = (
        ("crowded tile", np.concatenate([complete, knot]), 0.02, 224),
        ("long list", np.concatenate([complete, knot[:2000]]), 0.02, 224),
        ("wide discs", complete[:800], 0.12, 160),
        ("wide and narrow tiles", complete, 0.06, 224),
        ("large image", complete, 0.02, 544),
        ("one tile", complete[:400], 0.05, 16),
    )
    for name, comp, radius, size in cases:
        c = comp.astype(np.float64).mean(0).astype(np.float32)
        ccol, pcol = _colours(rng, len(comp), 0.25), _colours(rng, len(partial))
        for vc, pc in ((None, None), (ccol, pcol)):
            loss, grad = gp["POSE"].pose_loss_grad(torch.from_numpy(comp).cuda(), torch.from_numpy(c).cuda(), torch.from_numpy(params).cuda(),
                                                   torch.from_numpy(partial).cuda(), radius, size,
                                                   vert_col=None if vc is None else torch.from_numpy(vc).cuda(),
                                                   partial_col=None if pc is None else torch.from_numpy(pc).cuda())
            opts = oracle.pose_transform(comp, c, params)
            d1, d2, i1, i2 = oracle.chamfer_forward(opts[None], partial[None], 1)
            ref = oracle.splat_image(partial, radius, size, pc)
            lo, g = oracle.pose_full_loss_grad(comp, c, params, partial, d1[0], i1[0], d2[0], i2[0], radius, size, ref, vert_col=vc)
            np.testing.assert_allclose(loss.cpu().numpy(), lo, rtol=2e-4, atol=1e-5, err_msg=name)
            gg, go = grad.cpu().numpy().astype(np.float64), g.astype(np.float64)
            for sl in (slice(0, 6), slice(6, 9), slice(9, 10)):
                assert np.abs(gg[sl] - go[sl]).max() <= 2e-3 * np.abs(go[sl]).max() + 1e-6, (name, sl, gg[sl], go[sl])
            # a second call through the same scratch: the lists were handed back empty
            loss2, grad2 = gp["POSE"].pose_loss_grad(torch.from_numpy(comp).cuda(), torch.from_numpy(c).cuda(), torch.from_numpy(params).cuda(),
                                                     torch.from_numpy(partial).cuda(), radius, size,
                                                     vert_col=None if vc is None else torch.from_numpy(vc).cuda(),
                                                     partial_col=None if pc is None else torch.from_numpy(pc).cuda())
            assert torch.equal(loss, loss2) and torch.equal(grad, grad2), name


def test_full_loss_and_gradient_vs_oracle(gp, oracle, render_blend):
    """compute_loss_function as a whole (mask + 3 cd + ortho): loss terms and the 10-vector
    gradient against the oracle (whose loss is pinned to the reference's own code and whose gradient
    to torch autograd), white clouds and coloured clouds with a dark third."""
    torch = gp["torch"]
    complete, partial, _ = _shape(3, 3000)
    params = np.array([0.9, 0.1, -0.3, 0.05, 1.1, 0.2, 0.02, -0.01, 0.03, math.log(0.8)], np.float32)
    c = complete.astype(np.float64).mean(0).astype(np.float32)
    C, P, PR, CT = (torch.from_numpy(x).cuda() for x in (complete, partial, params, c))
    rng = np.random.default_rng(8)
    ccol, pcol = _colours(rng, len(complete), 0.33), _colours(rng, len(partial))
    seen = []
    for radius, size, vc, pc in ((0.02, 224, None, None), (0.03, 128, None, None), (0.02, 224, ccol, pcol), (0.03, 96, ccol, pcol)):
        loss, grad = gp["POSE"].pose_loss_grad(C, CT, PR, P, radius, size, vert_col=None if vc is None else torch.from_numpy(vc).cuda(),
                                               partial_col=None if pc is None else torch.from_numpy(pc).cuda())
        opts = oracle.pose_transform(complete, c, params)
        d1, d2, i1, i2 = oracle.chamfer_forward(opts[None], partial[None], 1)
        ref = oracle.splat_image(partial, radius, size, pc)
        lo, g = oracle.pose_full_loss_grad(complete, c, params, partial, d1[0], i1[0], d2[0], i2[0], radius, size, ref, vert_col=vc)
        np.testing.assert_allclose(loss.cpu().numpy(), lo, rtol=2e-4, atol=1e-5)
        lo_cd, g_cd = oracle.pose_loss_grad(complete, c, params, partial, d1[0], i1[0], d2[0], i2[0])
        gg, go = grad.cpu().numpy().astype(np.float64), g.astype(np.float64)
        # the mask term must carry weight here, or the comparison says nothing about it.  (Pulsar's blend on WHITE clouds: the
        # image is 1 wherever a disc covers a pixel and 0 elsewhere -- a hard rim, every covered pixel's soft mask saturated in
        # fp32 -- so the mask term is piecewise constant in the pose and its gradient exactly 0; with colours the softmax
        # weights of overlapping discs carry it.)
        if not (render_blend == 1 and vc is None):
            assert np.abs(go - g_cd).max() > 0.05 * np.abs(go).max()
        else:
            assert lo[3] > 0.0
        for sl in (slice(0, 6), slice(6, 9), slice(9, 10)):
            assert np.abs(gg[sl] - go[sl]).max() <= 2e-3 * np.abs(go[sl]).max(), (sl, gg[sl], go[sl])
        seen.append((float(loss[3]), gg))
    # colours change the loss and its gradient (same geometry, same radius and size: cases 0 and 2)
    assert abs(seen[0][0] - seen[2][0]) > 1e-2 and np.abs(seen[0][1] - seen[2][1]).max() > 1e-2 * np.abs(seen[0][1]).max()


def test_dark_points_drop_out_of_the_mask(gp, oracle):
    """the reference's soft mask is a LUMINANCE threshold (diff_obj_pose.py:273-277), so
    points darker than 0.1 leave it.  Same posed geometry, once bright, once with its x > 0 half at 5 %
    brightness: the loss against a bright reference must rise, and exactly as the oracle says."""
    torch = gp["torch"]
    complete, partial, _ = _shape(6, 3000)
    params = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, math.log(0.9)], np.float32)
    c = complete.astype(np.float64).mean(0).astype(np.float32)
    bright = np.full((len(complete), 3), 0.9, np.float32)
    half = bright.copy()
    half[complete[:, 0] > c[0]] = 0.045
    pcol = np.full((len(partial), 3), 0.9, np.float32)
    C, P, PR, CT = (torch.from_numpy(x).cuda() for x in (complete, partial, params, c))
    out = {}
    for name, col in (("bright", bright), ("half", half)):
        loss, grad = gp["POSE"].pose_loss_grad(C, CT, PR, P, 0.02, 224, vert_col=torch.from_numpy(col).cuda(),
                                               partial_col=torch.from_numpy(pcol).cuda())
        opts = oracle.pose_transform(complete, c, params)
        d1, d2, i1, i2 = oracle.chamfer_forward(opts[None], partial[None], 1)
        lo, g = oracle.pose_full_loss_grad(complete, c, params, partial, d1[0], i1[0], d2[0], i2[0], 0.02, 224,
                                           oracle.splat_image(partial, 0.02, 224, pcol), vert_col=col)
        np.testing.assert_allclose(loss.cpu().numpy(), lo, rtol=2e-4, atol=1e-5)
        out[name] = float(loss[3])
    assert out["half"] > out["bright"] + 0.2, out


def test_pose_loop_full_objective(gp, oracle, render_blend):
    """object_pose_optimization with radius / render_size live (the reference's call: radius 0.02,
    224 x 224), white and coloured clouds: the early loss history tracks the oracle's loop, the same start
    wins, and the result differs from the Chamfer-only run."""
    torch = gp["torch"]
    complete, partial, Rt = _shape(9, 1200)
    C, P = torch.from_numpy(complete).cuda(), torch.from_numpy(partial).cuda()
    rng = np.random.default_rng(12)
    for ccol, pcol in ((None, None), (_colours(rng, len(complete), 0.25), _colours(rng, len(partial)))):
        kw = {} if ccol is None else dict(complete_col=torch.from_numpy(ccol).cuda(), partial_col=torch.from_numpy(pcol).cuda())
        T, hist, bp = gp["POSE"].object_pose_optimization(C, P, radius=0.02, lr=0.01, iters=60, render_size=224,
                                                          return_history=True, **kw)
        oT, ohist, obp = oracle.pose_optimize(complete, partial, lr=0.01, iters=60, starts=4, radius=0.02, size=224,
                                              complete_col=ccol, partial_col=pcol)
        assert hist.shape == (4, 61) and np.isfinite(hist).all()
        np.testing.assert_allclose(hist[:, :10], ohist[:, :10], rtol=5e-3)
        best = int(np.argmin(ohist.min(1)))
        assert int(np.argmin(hist.min(1))) == best
        # the winning start ends where the oracle's does; the losing starts (rotated by 90 / 180 / 270
        # degrees) wander: the loss jumps by 100 / P whenever a pixel's soft mask saturates (fp32
        # sigmoid + BCE clamp, as in the reference), so late trajectories are not comparable
        np.testing.assert_allclose(hist.min(1)[best], ohist.min(1)[best], rtol=0.02 if render_blend == 0 else 0.10)      # (Pulsar's hard rims: a pixel entering a silhouette moves the loss by 100 / P at once)
        assert T[3].tolist() == [0, 0, 0, 1]
    Tc, hc, _ = gp["POSE"].object_pose_optimization(C, P, radius=0.02, lr=0.01, iters=60, return_history=True, cd_only=True)
    assert np.abs(hist[:, 0] - hc[:, 0]).min() > 1e-3        # the mask term is in the loss


def test_pose_optimisation_loop(gp, oracle):
    torch = gp["torch"]
    complete, partial, Rt = _shape(9, 1200)
    T, hist, bp = gp["POSE"].object_pose_optimization(torch.from_numpy(complete).cuda(), torch.from_numpy(partial).cuda(),
                                                      radius=0.02, lr=0.01, iters=200, return_history=True, cd_only=True)
    oT, ohist, obp = oracle.pose_optimize_cd(complete, partial, lr=0.01, iters=200, starts=4)
    assert hist.shape == (4, 201)
    assert int(np.argmin(hist.min(1))) == int(np.argmin(ohist.min(1)))
    np.testing.assert_allclose(hist[:, :20], ohist[:, :20], rtol=2e-3)     # early steps track closely
    np.testing.assert_allclose(hist.min(1), ohist.min(1), rtol=0.02)
    np.testing.assert_allclose(T, oT, atol=1e-2)
    s = np.cbrt(np.linalg.det(T[:3, :3].astype(np.float64)))
    assert abs(s - 0.9) < 0.03
    np.testing.assert_allclose(T[:3, :3] / s, Rt, atol=0.03)
    np.testing.assert_allclose(T[:3, 3], [0.02, -0.01, 0.015], atol=0.01)
    assert T[3].tolist() == [0, 0, 0, 1]


def test_pose_loop_early_stop(gp, oracle):
    """diff_obj_pose.py:529-556: a start leaves its loop once 300 steps in a row have not improved its best loss (the
    optimizer step of that iteration has been taken).  Never fires at reg()'s iters = 200; with lr = 0 every step after the
    first fails to improve: iterations 0 .. 301 run, 302 .. 400 do not (NaN in the history), in the library and the oracle."""
    torch = gp["torch"]
    complete, partial, _ = _shape(9, 600)
    T, hist, bp = gp["POSE"].object_pose_optimization(torch.from_numpy(complete).cuda(), torch.from_numpy(partial).cuda(),
                                                      radius=0.02, lr=0.0, iters=400, return_history=True, cd_only=True)
    oT, ohist, obp = oracle.pose_optimize_cd(complete, partial, lr=0.0, iters=400, starts=4)
    assert hist.shape == (4, 401)
    assert np.isfinite(hist[:, :302]).all() and np.isnan(hist[:, 302:]).all()
    assert np.isfinite(ohist[:, :302]).all() and np.isnan(ohist[:, 302:]).all()
    np.testing.assert_allclose(hist[:, :302], ohist[:, :302], rtol=1e-4)
    np.testing.assert_allclose(T, oT, atol=1e-5)
    # a normal run (the loss keeps improving) is not cut short: iters = 320 > patience
    T2, h2, _ = gp["POSE"].object_pose_optimization(torch.from_numpy(complete).cuda(), torch.from_numpy(partial).cuda(),
                                                    radius=0.02, lr=0.01, iters=320, return_history=True, cd_only=True)
    best = int(np.argmin(np.nanmin(h2, 1)))
    assert np.isfinite(h2[best]).all()


def test_pose_loop_full_size_property(gp):
    """BASELINE config 5 size (32768 points): registration brings the one-sided
    Chamfer distance of the partial cloud (exactly 0 at the true pose here: the
    partial cloud is a noiseless subset) from its starting value down to below 1 % of
    the object's extent, and recovers scale / rotation / translation."""
    torch = gp["torch"]
    from genpc_amd.utils.loss_util import Completionloss
    complete, partial, Rt = _shape(11, 32768)
    C, P = torch.from_numpy(complete).cuda(), torch.from_numpy(partial).cuda()
    T = gp["POSE"].object_pose_optimization(C, P, lr=0.01, iters=200, cd_only=True)
    c = C.mean(0)
    Tt = torch.from_numpy(T).cuda()
    aligned = (C - c) @ Tt[:3, :3].T + c + Tt[:3, 3]
    cl = Completionloss("cd_l1")
    got = cl.chamfer_partial_l1(P[None], aligned[None].contiguous()).item()
    truth = ((C - c) * 0.9) @ torch.from_numpy(Rt.astype(np.float32)).cuda().T + c + torch.tensor([0.02, -0.01, 0.015]).cuda()
    ref = cl.chamfer_partial_l1(P[None], truth[None].contiguous()).item()
    start = cl.chamfer_partial_l1(P[None], ((C - c) * 0.75 + c)[None].contiguous()).item()
    assert ref < 1e-6 and got < 0.01 and got < 0.25 * start, (got, ref, start)
    s = np.cbrt(np.linalg.det(T[:3, :3].astype(np.float64)))
    assert abs(s - 0.9) < 0.03
    # 201 Adam steps at lr 0.01 stop a few degrees short of the 12 degree truth at
    # this density (a property of the reference's schedule, not of the kernels)
    np.testing.assert_allclose(T[:3, :3] / s, Rt, atol=0.08)
    np.testing.assert_allclose(T[:3, 3], [0.02, -0.01, 0.015], atol=0.02)


def test_pose_loop_batched_equals_singles(gp):
    """B scans in lock-step (one batched NN launch per Adam step) give the same transforms as B
    separate runs.  Chamfer-only objective: fp64 reductions are atomics, last-bit noise only.  Full
    objective: the splat sums its list in an order that varies from run to run and the loss jumps
    by 100 / P when a soft-mask pixel saturates, so only the first steps are comparable."""
    torch = gp["torch"]
    cs, ps = [], []
    for seed in (9, 10, 11):
        c, p, _ = _shape(seed, 1500)
        cs.append(c)
        ps.append(p[:700])
    C = torch.from_numpy(np.stack(cs)).cuda()
    P = torch.from_numpy(np.stack(ps)).cuda()
    Tb, hb, _ = gp["POSE"].object_pose_optimization(C, P, lr=0.01, iters=60, return_history=True, cd_only=True)
    assert Tb.shape == (3, 4, 4) and hb.shape == (3, 4, 61)
    Tf, hf, _ = gp["POSE"].object_pose_optimization(C, P, radius=0.02, lr=0.01, iters=20, return_history=True)
    for i in range(3):
        Ti, hi, _ = gp["POSE"].object_pose_optimization(C[i], P[i], lr=0.01, iters=60, return_history=True, cd_only=True)
        np.testing.assert_allclose(hb[i][:, :10], hi[:, :10], rtol=1e-5)
        np.testing.assert_allclose(Tb[i], Ti, atol=2e-3)
        _, hfi, _ = gp["POSE"].object_pose_optimization(C[i], P[i], radius=0.02, lr=0.01, iters=20, return_history=True)
        np.testing.assert_allclose(hf[i][:, :5], hfi[:, :5], rtol=2e-3)


def test_zbuffer_visibility_and_viewpoint_select(gp, oracle):
    """f3, the cheaper z-buffer ranking (the exact operator is tested in test_gpu_hpr.py): bit-exact vs the oracle's restatement of the
    same definition; on a closed surface about half the points face any camera; the
    selected view of a hemisphere shell looks at its open side's opposite."""
    torch = gp["torch"]
    rng = np.random.default_rng(2)
    u = rng.standard_normal((20000, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    sphere = (u * 0.4).astype(np.float32)
    dp = gp["dp"]
    uv, depth, _ = dp.getUvs(dp.cameras, torch.from_numpy(sphere).cuda(), want_transformed=False)
    vis, cnt = dp.getVisiblePointsZBuffer(None, uvs=uv, depths=depth, tol=2e-4, res=256, point_size=3)
    ovis, ocnt = oracle.zbuffer_visibility(uv.cpu().numpy(), depth.cpu().numpy(), 256, 2e-4, 3)
    np.testing.assert_array_equal(vis.cpu().numpy(), ovis)
    np.testing.assert_array_equal(cnt.cpu().numpy(), ocnt)
    # every visible point of a sphere faces the camera, and the far side is hidden
    eyes = gp["DP"].fibonacci_sphere(16, 1.6)
    facing = (sphere @ eyes[3]) > 0
    v3 = vis[3].cpu().numpy()
    # (points near the limb are occluded by their nearer neighbours' stamps: ~half of the facing side survives)
    assert v3[facing].mean() > 0.4 and v3[~facing].mean() < 0.03, (v3[facing].mean(), v3[~facing].mean())
    # viewpoint_select = FPS subsample -> visibility from all cameras -> arg-max of the counts
    from genpc_amd.fps import fps_sampling
    cap = torch.from_numpy(sphere[sphere[:, 1] > 0.15]).cuda()
    gp["cfg"].downsample_num = 3000
    gp["cfg"].cam_res = 128
    best = dp.viewpoint_select(cap, zbuffer=True)
    sub = cap[fps_sampling(cap, 3000).long()]
    _, counts = dp.getVisiblePointsZBuffer(sub, cams=dp.cameras, tol=1e-4)
    assert best == int(torch.argmax(counts)) and int(counts.max()) > 1500


def test_get_uvs_fuzz(gp, oracle):
    """40 random shapes: 1 .. 70000 points, 1 .. 200 cameras at random eyes (incl. points behind a camera and far
    off-axis), scales 1e-2 .. 1e2, rescale on and off, paddings 0 .. 0.3 -- uv / depth / transformed points are
    the oracle's, bit for bit (NaN where the oracle has NaN)."""
    torch = gp["torch"]
    DP = gp["DP"]
    rng = np.random.default_rng(99)
    for case in range(40):
        n = int(rng.integers(2, 70001)) if case % 4 else int(rng.integers(2, 70))
        c = int(rng.integers(1, 201)) if case % 3 else int(rng.integers(1, 4))
        scale = 10.0 ** rng.uniform(-2, 2)
        xyz = ((rng.random((n, 3)) - 0.5) * scale).astype(np.float32)
        eyes = rng.normal(size=(c, 3))
        eyes *= (scale * rng.uniform(0.3, 4.0, size=(c, 1))) / np.linalg.norm(eyes, axis=1, keepdims=True)
        views = np.stack([DP.look_at(e, np.zeros(3), DP.calculate_up_vector(e, np.zeros(3))) for e in eyes]).astype(np.float32)
        rescale = bool(case & 1)
        padding = float(rng.choice([0.0, 0.15, 0.3]))
        uv, depth, tr = gp["dp"].getUvs(torch.from_numpy(views).cuda(), torch.from_numpy(xyz).cuda(), rescale=rescale, padding=padding)
        ouv, od, otr, _ = oracle.get_uvs(views, gp["dp"].focal, xyz, rescale=rescale, padding=padding)
        assert np.array_equal(uv.cpu().numpy(), ouv, equal_nan=True), (case, n, c)
        assert np.array_equal(depth.cpu().numpy(), od, equal_nan=True), (case, n, c)
        assert np.array_equal(tr.cpu().numpy(), otr, equal_nan=True), (case, n, c)


def test_get_uvs_operands_outside_the_fast_division_range(gp, oracle):
    """The write pass divides with csrc/fastdiv.h inside [2^-50, 2^50] and with the compiler's division outside
    (per wave and camera); the box pass rescans everything exactly when its approximate pass meets a non-finite
    quotient.  Operands built to leave the range: zeros (points on a camera axis, a point at the box centre),
    a point on the camera plane (w = 0 -> infinite quotients), huge and tiny scenes."""
    torch = gp["torch"]
    focal = gp["dp"].focal
    g = np.linspace(-0.5, 0.5, 21, dtype=np.float32)
    grid = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)          # symmetric, contains the origin and the axes
    axis_cam = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -1.6]], np.float32)       # looks down -z from (0, 0, 1.6)
    tilted = gp["dp"].cameras[:3].cpu().numpy().reshape(-1, 12)
    cases = [("zeros", grid, np.concatenate([axis_cam, tilted])),
             ("camera plane", np.concatenate([grid, np.array([[0.25, 0.125, 1.6]], np.float32)]), axis_cam),
             ("huge", grid * np.float32(2.0 ** 60), np.concatenate([axis_cam, tilted]) * np.array([1, 1, 1, 2.0 ** 60] * 3, np.float32)),
             ("tiny", grid * np.float32(2.0 ** -60), np.concatenate([axis_cam, tilted]) * np.array([1, 1, 1, 2.0 ** -60] * 3, np.float32))]
    for name, xyz, views in cases:
        for rescale in (True, False):
            uv, depth, tr = gp["dp"].getUvs(torch.from_numpy(views).cuda(), torch.from_numpy(xyz).cuda(), rescale=rescale, padding=0.15)
            ouv, od, otr, _ = oracle.get_uvs(views, focal, xyz, rescale=rescale, padding=0.15)
            assert np.array_equal(tr.cpu().numpy(), otr, equal_nan=True), (name, rescale)
            assert np.array_equal(depth.cpu().numpy(), od, equal_nan=True), (name, rescale)
            assert np.array_equal(uv.cpu().numpy(), ouv, equal_nan=True), (name, rescale)


def test_paint_and_gather_fuzz(gp, oracle):
    """30 random cases of uvToPixels -> paintPixels (collisions: the highest point index wins) -> gather_colors:
    1 .. 50000 points, resolutions 8 .. 512, point sizes 1 .. 4, uv partly out of range."""
    torch = gp["torch"]
    rng = np.random.default_rng(123)
    for case in range(30):
        n = int(rng.integers(1, 50001)) if case % 3 else int(rng.integers(1, 40))
        res = int(rng.choice([8, 31, 64, 256, 512]))
        ps = int(rng.integers(1, 5))
        uv = (rng.random((n, 2), dtype=np.float32) * 1.2 - 0.1).astype(np.float32)
        pix = gp["dp"].uvToPixels(torch.from_numpy(uv).cuda(), res)
        opix = oracle.uv_to_pixels(uv, res)
        np.testing.assert_array_equal(pix.cpu().numpy(), opix)
        col = rng.random((n, 3), dtype=np.float32)
        img = torch.zeros(3, res, res, device="cuda")
        out = gp["dp"].paintPixels(img, pix, torch.from_numpy(col).cuda(), ps)
        oout, oimg = oracle.paint_pixels(res, opix, col, ps)
        np.testing.assert_array_equal(out.cpu().numpy(), oout, err_msg="case %d" % case)
        np.testing.assert_array_equal(img.cpu().numpy(), oimg, err_msg="case %d" % case)
        # ... and back: every point's colour from the flipped image (ScaleAdapter.py:57-66).  Many points on a small image
        # take the interleaved-copy gather (csrc/project.hip: one 16-byte read per point), few points the three planar reads.
        from genpc_amd import _lib
        got = torch.empty(n, 3, device="cuda")
        rc = _lib.on_device_of(out, _lib.lib.genpc_gather_colors, n, _lib.ptr(pix), _lib.ptr(out), 3, res, res, _lib.ptr(got))
        assert rc == 1
        np.testing.assert_array_equal(got.cpu().numpy(), oracle.gather_colors(opix, oout), err_msg="case %d gather" % case)


@pytest.mark.parametrize("n,res,ps", [(300000, 1000, 1), (280000, 512, 2), (262144, 130, 4)])
def test_paint_many_points_takes_the_tile_elections(gp, oracle, n, res, ps):
    """paintPixels with many points (csrc/project.hip: from 262144 points on, the owners are elected per 64 x 64-pixel tile in LDS
    after a counting sort of the points by tile): img, the flipped out and the owners equal the oracle's, collisions and stamps
    across tile borders included; uv partly out of range."""
    torch = gp["torch"]
    rng = np.random.default_rng(n + res)
    uv = (rng.random((n, 2), dtype=np.float32) * 1.1 - 0.05).astype(np.float32)
    uv[:1000] = uv[1000:2000]                       # exact collisions: the highest index wins
    pix = gp["dp"].uvToPixels(torch.from_numpy(uv).cuda(), res)
    opix = oracle.uv_to_pixels(uv, res)
    np.testing.assert_array_equal(pix.cpu().numpy(), opix)
    col = rng.random((n, 3), dtype=np.float32)
    base = rng.random((3, res, res), dtype=np.float32)
    img = torch.from_numpy(base.copy()).cuda()
    out = gp["dp"].paintPixels(img, pix, torch.from_numpy(col).cuda(), ps)
    oout, oimg = oracle.paint_pixels(res, opix, col, ps, img=base.copy())
    np.testing.assert_array_equal(out.cpu().numpy(), oout)
    np.testing.assert_array_equal(img.cpu().numpy(), oimg)
