"""render_points_ragged on the device (csrc/render_grad.hip: genpc_render_points_ragged, genpc_render_points_ragged_backward;
genpc_amd.optim_registration.diff_obj_pose): every element's image, planes and gradients against the equal-size entry points on
that element alone -- bit for bit --, determinism, exact +0 rows and edge lists, the autograd layer with its cameras, the modules
on top, and the refusals.  The shapes are the smallest at which the kernels can go wrong: the backward gather takes 32 points a
block, the projection 256, xcd_block branches on multiples of 8 elements."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 31, 32, 33, 255, 257, 2451)
LISTS = {1: (257,), 3: (33, 0, 2451), 8: (2451, 0, 1, 31, 32, 33, 255, 257), 9: (31, 257, 0, 33, 2451, 1, 255, 32, 33)}


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib
    from genpc_amd.optim_registration import diff_obj_pose as P
    return dict(torch=torch, lib=_lib, P=P)


def _dev(env, a):
    return None if a is None else env["torch"].from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _cloud(seed, n, spread=0.9, depth=0.3):
    rng = np.random.default_rng(seed)
    pts = np.c_[(rng.random((n, 2)) - 0.5) * spread, (rng.random(n) - 0.5) * depth].astype(np.float32)
    return pts, (0.1 + 0.85 * rng.random((n, 3))).astype(np.float32)


def _upstream(env, seed, s, S):
    return _dev(env, np.random.default_rng(seed).random((s, S, S, 3)) - 0.5)


def _pack(env, clouds):
    """list of device [n_j,3] -> (packed [T,3], offsets)"""
    torch = env["torch"]
    off = [0]
    for c in clouds:
        off.append(off[-1] + c.shape[0])
    return (torch.cat(clouds, dim=0).contiguous() if clouds else torch.empty(0, 3, device="cuda")), off


def _ragged(env, pts, cols, radii, S, blend, G, want_col=True):
    """one ragged forward and backward on lists of device tensors -> (img [s,S,S,3], planes [s,5,S*S], grad_pts [T,3], grad_col or None, off)"""
    P = env["P"]
    p, off = _pack(env, pts)
    c = None if cols is None else _pack(env, cols)[0]
    img, planes = P.render_points_ragged_forward(p, off, c, list(radii), S, blend)
    gp, gc = P.render_points_ragged_backward(p, off, c, list(radii), S, blend, planes, G, want_col)
    return img, planes, gp, gc, off


def _alone(env, pts, col, radius, S, blend, G, want_col=True):
    """the equal-size entry points on one element alone, b = 1 -> (img [S,S,3], planes [5,S*S], grad_pts [n,3], grad_col or None)"""
    P = env["P"]
    p, c = pts[None].contiguous(), None if col is None else col[None].contiguous()
    img, planes = P.render_points_forward(p, c, radius, S, blend)
    gp, gc = P.render_points_backward(p, c, radius, S, blend, planes, G[None].contiguous(), want_col)
    return img[0], planes[0], gp[0], None if gc is None else gc[0]


def _check_list(env, pts, cols, radii, S, blend, G, want_col=True, what=""):
    """the ragged call's element j == the equal-size call on element j alone, in every output"""
    img, planes, gp, gc, off = _ragged(env, pts, cols, radii, S, blend, G, want_col)
    assert img.shape == (len(pts), S, S, 3) and planes.shape == (len(pts), 5, S * S) and gp.shape == (off[-1], 3)
    assert (gc is None) == (not want_col)
    for j in range(len(pts)):
        i1, p1, g1, k1 = _alone(env, pts[j], None if cols is None else cols[j], radii[j], S, blend, G[j], want_col)
        tag = (what, j, pts[j].shape[0], S, blend)
        assert _same(img[j], i1), ("image",) + tag
        assert _same(planes[j], p1), ("planes",) + tag
        assert _same(gp[off[j]:off[j + 1]], g1), ("grad_pts",) + tag
        if want_col:
            assert _same(gc[off[j]:off[j + 1]], k1), ("grad_col",) + tag
    return img, planes, gp, gc


def _list_of(env, sizes, seed):
    clouds = [_cloud(seed + 17 * j, n, 0.5 + 0.05 * (j % 7), 0.2) for j, n in enumerate(sizes)]
    return [_dev(env, p).reshape(-1, 3) for p, _ in clouds], [_dev(env, c).reshape(-1, 3) for _, c in clouds]


# ------------------------------------------------------------------------------------------------ 1. per-element bits

@pytest.mark.parametrize("blend", (1, 0))
@pytest.mark.parametrize("s", sorted(LISTS))
def test_every_element_is_the_equal_size_call_on_it_alone(env, s, blend):
    sizes = LISTS[s]
    assert len(sizes) == s and set(sizes) <= set(SIZES) and (s < 8 or set(sizes) == set(SIZES))          # (8 and 9 hold every size)
    pts, cols = _list_of(env, sizes, 100 * s)
    radii = [0.02 + 0.004 * j for j in range(s)]
    drawn = 0.0
    for S in (64, 96):
        G = _upstream(env, s + S, s, S)
        img, _, gp, gc = _check_list(env, pts, cols, radii, S, blend, G, True, "coloured")
        _check_list(env, pts, cols, radii, S, blend, G, False, "coloured, no grad_col")
        _check_list(env, pts, None, radii, S, blend, G, True, "white")
        _check_list(env, pts, None, radii, S, blend, G, False, "white, no grad_col")
        drawn = max(drawn, float(img.abs().max()), 0.0)
        assert float(gp.abs().max()) > 0 and float(gc.abs().max()) > 0
    assert drawn > 0


@pytest.mark.parametrize("blend", (1, 0))
def test_the_same_points_with_two_radii(env, blend):
    p, c = _cloud(3, 700, 0.6, 0.2)
    pts, cols = [_dev(env, p)] * 2, [_dev(env, c)] * 2
    S, r = 64, 0.015
    G = _upstream(env, 4, 2, S)
    img, planes, gp, gc = _check_list(env, pts, cols, [r, 2 * r], S, blend, G)
    assert not _same(img[0], img[1]) and not _same(gp[:700], gp[700:])


@pytest.mark.parametrize("blend", (1, 0))
def test_crowded_tile_and_full_scan_inside_a_ragged_call(env, blend):
    """Element 0: 1500 small discs over one tile (more than kSplatCap = 1024 entries in that tile's list: the list is drawn in
    several fills).  Element 1: discs of more than 16 pixels' radius, each over more than four tiles: they are in no list and
    poison their tiles' counters, so the splat's full scan runs.  Element 2: an ordinary cloud behind them."""
    rng = np.random.default_rng(21)
    S = 96
    crowd = np.c_[0.01 + 0.004 * (rng.random((1500, 2)) - 0.5), 0.05 * (rng.random(1500) - 0.5)].astype(np.float32)
    # the crowd projects into one tile (columns 48 .. 63 of 96)
    u = 48.0 * (1 + 4 * crowd[:, 0] / (3 - crowd[:, 2]))
    assert u.min() > 48.2 and u.max() < 63.0 and len(crowd) > 1024
    big, bigc = _cloud(22, 300, 0.5, 0.2)
    rest, restc = _cloud(23, 500, 0.7, 0.2)
    pts = [_dev(env, crowd), _dev(env, big), _dev(env, rest)]
    cols = [_dev(env, 0.1 + 0.85 * rng.random((1500, 3))), _dev(env, bigc), _dev(env, restc)]
    radii = [0.004, 0.3, 0.02]                      # 0.3 world units at depth ~3: rho = 48 * 4 * 0.3 / 3 = 19 pixels
    G = _upstream(env, 24, 3, S)
    _check_list(env, pts, cols, radii, S, blend, G)
    _check_list(env, pts[::-1], cols[::-1], radii[::-1], S, blend, G)


@pytest.mark.parametrize("blend", (1, 0))
def test_the_first_size_without_tile_lists(env, blend):
    """513 x 513: 33 x 33 tiles, more than the 1024 a block's histogram holds -- no lists, every tile by the full scan"""
    S = 513
    pts, cols = _list_of(env, (257, 33), 31)
    G = _upstream(env, 32, 2, S)
    img, _, gp, _ = _check_list(env, pts, cols, [0.02, 0.03], S, blend, G)
    assert float(img.abs().max()) > 0 and float(gp.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 2. determinism

@pytest.mark.parametrize("blend", (1, 0))
def test_the_same_bytes_every_time_everywhere(env, blend):
    torch, P = env["torch"], env["P"]
    sizes = LISTS[9]
    s, S = len(sizes), 64
    pts, cols = _list_of(env, sizes, 900)
    radii = [0.02 + 0.004 * j for j in range(s)]
    G = _upstream(env, 41, s, S)
    img, planes, gp, gc, off = _ragged(env, pts, cols, radii, S, blend, G)
    again = _ragged(env, pts, cols, radii, S, blend, G)
    assert all(_same(a, b) for a, b in zip((img, planes, gp, gc), again[:4]))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        there = _ragged(env, pts, cols, radii, S, blend, G)
    side.synchronize()
    assert all(_same(a, b) for a, b in zip((img, planes, gp, gc), there[:4]))
    # the list reversed: every element's bytes are where the element now stands
    rimg, rplanes, rgp, rgc, roff = _ragged(env, pts[::-1], cols[::-1], radii[::-1], S, blend, torch.flip(G, dims=(0,)).contiguous())
    for j in range(s):
        k = s - 1 - j
        assert _same(rimg[k], img[j]) and _same(rplanes[k], planes[j])
        assert _same(rgp[roff[k]:roff[k + 1]], gp[off[j]:off[j + 1]]) and _same(rgc[roff[k]:roff[k + 1]], gc[off[j]:off[j + 1]])
    # the list packed as (points, offsets), through the public operation
    p, o = _pack(env, pts)
    c, _ = _pack(env, cols)
    a = P.render_points_ragged(pts, cols, radii, S, blend=blend)
    b = P.render_points_ragged((p, o), (c, o), radii, S, blend=blend)
    b2 = P.render_points_ragged((p, torch.tensor(o, dtype=torch.int64)), (c, o), radii, S, blend=blend)
    assert _same(a, img) and _same(b, img) and _same(b2, img)


# ------------------------------------------------------------------------------------------------ 3. exact +0 rows, edge lists

@pytest.mark.parametrize("blend", (1, 0))
def test_exact_zero_rows_and_empty_elements(env, blend):
    torch, P = env["torch"], env["P"]
    S = 64
    a, ac = _cloud(51, 300, 0.6, 0.2)
    b, bc = _cloud(52, 257, 0.6, 0.2)
    a[7] = (0.0, 0.0, 10.0)              # behind the eye
    a[100] = (np.nan, 0.1, 0.0)
    a[299] = (0.1, np.inf, 0.0)
    b[0] = (0.0, -np.inf, 0.2)
    b[256] = (0.0, 0.0, -2.5)            # beyond zfar
    empty = np.zeros((0, 3), np.float32)
    pts = [_dev(env, a), _dev(env, empty).reshape(0, 3), _dev(env, b)]
    cols = [_dev(env, ac), _dev(env, empty).reshape(0, 3), _dev(env, bc)]
    G = _upstream(env, 53, 3, S)
    img, planes, gp, gc = _check_list(env, pts, cols, [0.03, 0.02, 0.025], S, blend, G)
    for row in (7, 100, 299, 300 + 0, 300 + 256):
        assert not _bits(gp[row]).any() and not _bits(gc[row]).any(), row          # +0: no bit set, the sign bit included
    assert float(gp[:300].abs().max()) > 0 and float(gp[300:].abs().max()) > 0 and torch.isfinite(gp).all() and torch.isfinite(gc).all()
    # the empty element between the two: the background, i.e. what b = 1, n = 0 draws
    bg, bgp = P.render_points_forward(torch.empty(1, 0, 3, device="cuda"), None, 0.02, S, blend)
    assert _same(img[1], bg[0]) and _same(planes[1], bgp[0]) and not img[1].cpu().numpy().any()
    # a list of empty elements only: backgrounds, and a backward that has nothing to write
    e3 = [_dev(env, empty).reshape(0, 3)] * 3
    img0, planes0, gp0, gc0, off0 = _ragged(env, e3, e3, [0.02, 0.03, 0.04], S, blend, G)
    assert off0 == [0, 0, 0, 0] and gp0.shape == (0, 3) and gc0.shape == (0, 3)
    for j in range(3):
        assert _same(img0[j], bg[0]) and _same(planes0[j], bgp[0])
    out = P.render_points_ragged(e3, None, 0.02, S, blend=blend)
    assert _same(out, img0)


# ------------------------------------------------------------------------------------------------ 4. the autograd layer

def test_autograd_layer(env):
    torch, P = env["torch"], env["P"]
    S = 64
    sizes = (257, 0, 33, 500)
    radii = [0.03, 0.02, 0.04, 0.025]
    G = _upstream(env, 61, len(sizes), S)
    prev = P.render_tune(-1)
    try:
        for blend in (1, 0):
            pts, cols = _list_of(env, sizes, 600)
            _, planes, gp, gc, off = _ragged(env, pts, cols, radii, S, blend, G)
            lp = [p.clone().requires_grad_(True) for p in pts]
            lc = [c.clone().requires_grad_(True) for c in cols]
            img = P.render_points_ragged(lp, lc, radii, S, blend=blend)
            assert img.shape == (len(sizes), S, S, 3)
            (img * G).sum().backward()
            for j in range(len(sizes)):          # gradients reach every list element, and the colours
                assert lp[j].grad is not None and _same(lp[j].grad, gp[off[j]:off[j + 1]])
                assert lc[j].grad is not None and _same(lc[j].grad, gc[off[j]:off[j + 1]])
            # the packed form: one gradient for the packed points; colours that do not require grad get none
            pp, o = _pack(env, pts)
            pc, _ = _pack(env, cols)
            pp = pp.clone().requires_grad_(True)
            (P.render_points_ragged((pp, o), (pc, o), radii, S, blend=blend) * G).sum().backward()
            assert _same(pp.grad, gp) and pc.grad is None
            # blend=None: the thread's mode at forward time, whatever is set by the time of the backward
            P.render_tune(blend)
            p2 = [p.clone().requires_grad_(True) for p in pts]
            img2 = P.render_points_ragged(p2, cols, radii, S)
            assert _same(img2, img)
            P.render_tune(1 - blend)
            (img2 * G).sum().backward()
            assert all(_same(p2[j].grad, gp[off[j]:off[j + 1]]) for j in range(len(sizes)))
            P.render_tune(-1)
            # one radius for all; white
            p3 = [p.clone().requires_grad_(True) for p in pts]
            img3 = P.render_points_ragged(p3, None, 0.03, S, blend=blend)
            assert _same(img3[0], P.render_points(pts[0], None, 0.03, S, blend=blend))
            (img3[3] * G[3]).sum().backward()
            assert not _bits(p3[0].grad).any() and float(p3[3].grad.abs().max()) > 0
        with pytest.raises(RuntimeError, match="GPU tensors only"):
            P.render_points_ragged([torch.zeros(4, 3)])
        with pytest.raises(ValueError, match="sizes of clouds"):
            P.render_points_ragged(pts, cols[:-1] + [cols[0]], radii, S)
        with pytest.raises(ValueError, match="one float per cloud"):
            P.render_points_ragged(pts, None, radii[:2], S)
        with pytest.raises(ValueError, match="radius of cloud 1 must be positive"):
            P.render_points_ragged(pts, None, [0.01, 0.0, 0.01, 0.01], S)
        with pytest.raises(ValueError, match="blend"):
            P.render_points_ragged(pts, None, 0.01, S, blend=2)
    finally:
        P.render_tune(prev)


@pytest.mark.parametrize("blend", (1, 0))
def test_cameras(env, blend):
    torch, P = env["torch"], env["P"]
    S, r = 64, 0.03
    sizes = (257, 33, 500)
    pts, cols = _list_of(env, sizes, 700)
    G = _upstream(env, 71, len(sizes), S)
    lib_R, lib_T = torch.tensor(P._CAMERA_R), torch.tensor(P._CAMERA_T)
    # cameras=None against the library camera given explicitly (one for all, and one each): equal bits, forward and backward
    base_p = [p.clone().requires_grad_(True) for p in pts]
    base = P.render_points_ragged(base_p, cols, r, S, blend=blend)
    (base * G).sum().backward()
    for cams in ((lib_R, lib_T, 4.0), (lib_R[None].repeat(3, 1, 1), lib_T[None].repeat(3, 1), [4.0, 4.0, 4.0])):
        q = [p.clone().requires_grad_(True) for p in pts]
        img = P.render_points_ragged(q, cols, r, S, blend=blend, cameras=cams)
        assert _same(img, base)
        (img * G).sum().backward()
        assert all(_same(q[j].grad, base_p[j].grad) for j in range(len(sizes)))
    # signed-permutation cameras with focal 2, 4 and 8 against render_points on coordinates permuted in numpy, radius r f / 4
    Rp = torch.tensor([[0.0, 0.0, -1.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])          # X_view = (-y, z, -x)
    focals = [2.0, 4.0, 8.0]
    img = P.render_points_ragged(pts, cols, r, S, blend=blend, cameras=(Rp, torch.tensor([0.0, 0.0, 3.0]), focals))
    for j, f in enumerate(focals):
        x = pts[j].cpu().numpy()
        xv = np.stack([-x[:, 1], x[:, 2], -x[:, 0]], axis=1)
        mapped = np.stack([np.float32(-f / 4) * xv[:, 0], np.float32(f / 4) * xv[:, 1], -xv[:, 2]], axis=1).astype(np.float32)
        want = P.render_points(_dev(env, mapped), cols[j], r * f / 4, S, blend=blend)
        assert _same(img[j], want), f
        assert float(want.abs().max()) > 0
    # a general look-at camera against render_points(camera_points(...)); gradients to R and T present and finite
    Rl, Tl = P.look_at_view_transform([(1.2, 0.6, 2.6), (-0.8, 0.3, 2.9), (0.0, 0.0, 3.0)])
    Rl, Tl = Rl.cuda().requires_grad_(True), Tl.cuda().requires_grad_(True)
    fl = [3.0, 5.0, 4.0]
    q = [p.clone().requires_grad_(True) for p in pts]
    img = P.render_points_ragged(q, cols, r, S, blend=blend, cameras=(Rl, Tl, fl))
    for j in range(3):
        want = P.render_points(P.camera_points(pts[j], Rl[j].detach(), Tl[j].detach(), fl[j]), cols[j], r * fl[j] / 4, S, blend=blend)
        assert _same(img[j], want) and float(want.abs().max()) > 0
    (img * G).sum().backward()
    assert Rl.grad is not None and Tl.grad is not None and torch.isfinite(Rl.grad).all() and torch.isfinite(Tl.grad).all()
    assert float(Rl.grad.abs().max()) > 0 and float(Tl.grad.abs().max()) > 0 and all(float(t.grad.abs().max()) > 0 for t in q)
    with pytest.raises(ValueError, match="cameras"):
        P.render_points_ragged(pts, cols, r, S, cameras=(Rl, Tl))
    with pytest.raises(ValueError, match="focal"):
        P.render_points_ragged(pts, cols, r, S, cameras=(Rl, Tl, [4.0, 0.0, 4.0]))


# ------------------------------------------------------------------------------------------------ 5. the modules

@pytest.mark.parametrize("blend", (1, 0))
def test_modules(env, blend):
    torch, P = env["torch"], env["P"]
    S, r = 64, 0.03
    p, c = _cloud(81, 700, 0.6, 0.3)
    vp, vc = _dev(env, p), _dev(env, c)
    prev = P.render_tune(blend)
    try:
        ref, mask, R_cam, T_cam = P.render_reference_image(vp, vc, r, S, "cuda")
        refs, masks = P.render_reference_images(vp, vc, r, S, R_cam, T_cam)
        assert refs.shape == (1, S, S, 3) and masks.shape == (1, S, S) and _same(refs[0], ref) and _same(masks[0], mask)
        assert not refs.requires_grad
        init = P.get_init_rot("y", 30, "cuda")
        one = P.ObjectPoseOptim(vp, vc, r, S, "cuda", R_cam, T_cam, init)
        views = P.ObjectPoseOptimViews(vp, vc, r, S, "cuda", R_cam, T_cam, init)
        assert sorted(n for n, _ in views.named_parameters()) == sorted(n for n, _ in one.named_parameters())
        assert sorted(n for n, _ in views.named_buffers()) == sorted(n for n, _ in one.named_buffers())
        img1, R1, s1, pts1 = one(return_pts=True)
        imgv, Rv, sv, ptsv = views(return_pts=True)
        assert imgv.shape == (1, S, S, 3) and _same(imgv[0], img1) and _same(ptsv, pts1) and _same(Rv, R1) and float(img1.detach().abs().max()) > 0
        # three cameras: its images are render_points_ragged's of the posed cloud, and the pose gets a gradient from every view
        R3, T3 = P.look_at_view_transform([(0.0, 0.0, 3.0), (1.5, 0.5, 2.4), (-1.0, 1.0, 2.5)])
        f3 = [4.0, 3.0, 5.0]
        three = P.ObjectPoseOptimViews(vp, vc, r, S, "cuda", R3, T3, init, focal=f3)
        imgs, _, _, pts3 = three(return_pts=True)
        assert imgs.shape == (3, S, S, 3) and _same(pts3, pts1) and _same(imgs[0], img1)
        want = P.render_points_ragged([pts3.detach()] * 3, [vc] * 3, 1.1 * r, S, cameras=(R3, T3, f3))
        assert _same(imgs, want) and not _same(imgs[1], imgs[0]) and float(imgs[2].detach().abs().max()) > 0
        refs3, masks3 = P.render_reference_images(vp, vc, r, S, R3, T3, f3)
        assert refs3.shape == (3, S, S, 3) and masks3.shape == (3, S, S) and _same(refs3[0], ref)
        ((imgs - refs3) ** 2).sum().backward()
        for prm in (three.rot_6d, three.trans, three.log_scale):
            assert prm.grad is not None and torch.isfinite(prm.grad).all() and float(prm.grad.abs().max()) > 0
        assert tuple(three.R_cam.shape) == (3, 3, 3) and tuple(three.T_cam.shape) == (3, 3) and three.focal_length.tolist() == f3
    finally:
        P.render_tune(prev)


# ------------------------------------------------------------------------------------------------ 6. refusals, chunks

def test_refusals_touch_nothing(env):
    """-1 by name with nothing enqueued and nothing written: small valid buffers (large enough for the list the valid arguments
    describe) hold a sentinel that must still stand; a backward of a list without points returns 1 and writes nothing"""
    torch, lib = env["torch"], env["lib"]
    L, p = lib.lib, lib.ptr
    names = ("pts", "col", "img", "planes", "grad_img", "grad_pts", "grad_col")
    buf = {k: torch.full((512,), 7.25, device="cuda") for k in names}          # s = 2, 8 points, 4 x 4 pixels: at most 160 floats
    st = lib.stream_of(buf["pts"])
    ints = lambda v: (ctypes.c_int * len(v))(*v)
    floats = lambda v: (ctypes.c_float * len(v))(*v)
    vp = lambda a: None if a is None else ctypes.cast(a, ctypes.c_void_p)

    def fwd(s=2, off=(0, 3, 8), radius=(0.02, 0.03), size=4, blend=1, pts="pts", img="img"):
        o, r = None if off is None else ints(off), None if radius is None else floats(radius)
        return L.genpc_render_points_ragged(s, vp(o), p(buf.get(pts)), p(buf["col"]), vp(r), size, blend, p(buf.get(img)), p(buf["planes"]), st)

    def bwd(s=2, off=(0, 3, 8), radius=(0.02, 0.03), size=4, blend=1, pts="pts", planes="planes", grad_img="grad_img", grad_pts="grad_pts"):
        o, r = None if off is None else ints(off), None if radius is None else floats(radius)
        return L.genpc_render_points_ragged_backward(s, vp(o), p(buf.get(pts)), p(buf["col"]), vp(r), size, blend, p(buf.get(planes)),
                                                     p(buf.get(grad_img)), p(buf.get(grad_pts)), p(buf["grad_col"]), st)
    both = [(dict(s=0), "s must be positive"), (dict(s=-1), "s must be positive"),
            (dict(s=385, off=tuple(range(386)), radius=(0.02,) * 385), "more than 384 elements in one call"),
            (dict(off=None), "off is null"), (dict(radius=None), "radius is null"),
            (dict(off=(1, 3, 8)), "offsets must start at 0"), (dict(off=(0, 5, 3)), "offsets must ascend"),
            (dict(radius=(0.02, 0.0)), "the radius of every element must be positive (element 1)"),
            (dict(radius=(-1.0, 0.02)), "the radius of every element must be positive (element 0)"),
            (dict(radius=(0.02, float("nan"))), "the radius of every element must be positive (element 1)"),
            (dict(size=0), "size must be in 1 .. 8192"), (dict(size=8193), "size must be in 1 .. 8192"),
            (dict(blend=2), "blend must be 0 or 1"), (dict(blend=-1), "blend must be 0 or 1"),
            (dict(off=(0, 3, (1 << 28) + 1)), "off[s] and s * size * size must not exceed 2^28"),
            (dict(s=5, off=(0, 1, 2, 3, 4, 5), radius=(0.02,) * 5, size=8192), "off[s] and s * size * size must not exceed 2^28"),
            (dict(pts=None), "pts is null")]
    for kw, words in both + [(dict(img=None), "img is null")]:
        assert fwd(**kw) == -1, kw
        assert lib.last_error() == "genpc_render_points_ragged: " + words, kw
    for kw, words in both + [(dict(planes=None), "planes is null"), (dict(grad_img=None), "grad_img is null"), (dict(grad_pts=None), "grad_pts is null")]:
        assert bwd(**kw) == -1, kw
        assert lib.last_error() == "genpc_render_points_ragged_backward: " + words, kw
    assert bwd(off=(0, 0, 0), pts=None, planes=None, grad_img=None, grad_pts=None) == 1          # nothing to do, nothing written
    torch.cuda.synchronize()
    for k in names:
        assert bool((buf[k] == 7.25).all()), k


def test_a_list_longer_than_a_call_goes_in_chunks(env):
    torch, P = env["torch"], env["P"]
    assert P.RENDER_RAGGED_MAX_ELEMENTS == 384
    s, S, blend = 390, 16, 1
    rng = np.random.default_rng(91)
    sizes = [int(v) for v in rng.integers(0, 40, s)]
    sizes[383], sizes[384] = 33, 31          # either side of the cut
    pts, cols = _list_of(env, sizes, 950)
    radii = [0.03 + 0.0001 * j for j in range(s)]
    G = _upstream(env, 92, s, S)
    _check_list(env, pts, cols, radii, S, blend, G)
