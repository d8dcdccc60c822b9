"""render_points on the device (csrc/render_grad.hip, genpc_amd.optim_registration.diff_obj_pose): the forward against
genpc_splat_image's bits, the backward against tests/render_points_ref.py in float64 at the bars tests/render_points_cases.py
measured on the CPU, its exact zeros, determinism, the autograd layer, the refusals, and the layers above -- the reference's
objective composed in torch and its Adam loop -- against the oracle."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_points_cases as C          # noqa: E402
import render_points_ref as RP           # noqa: E402

pytestmark = pytest.mark.gpu


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


def _run(env, pts, col, radius, S, blend, G, want_col=True):
    """one cloud [n,3] through the forward and the backward -> (img, planes, grad_pts, grad_col) as device tensors of the batch of one"""
    P = env["P"]
    p, c = _dev(env, pts)[None], None if col is None else _dev(env, col)[None]
    img, planes = P.render_points_forward(p, c, radius, S, blend)
    gp, gc = P.render_points_backward(p, c, radius, S, blend, planes, _dev(env, G)[None], want_col)
    return img, planes, gp, gc


def _cloud(seed, n, spread=0.9, depth=0.3):
    rng = np.random.default_rng(seed)
    pts = np.c_[(rng.random((n, 2)) - 0.5) * spread, (rng.random(n) - 0.5) * depth].astype(np.float32)
    return pts, (0.1 + 0.85 * rng.random((n, 3))).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 6. forward

@pytest.mark.parametrize("blend", (1, 0))
def test_forward_is_splat_image(env, blend):
    torch, P = env["torch"], env["P"]
    prev = P.render_tune(blend)
    try:
        pts, col = _cloud(1, 3000)
        for c in (None, col):
            for S, radius in ((224, 0.02), (97, 0.035)):
                want = P.splat_image(_dev(env, pts), radius, S, _dev(env, c))
                img, planes = P.render_points_forward(_dev(env, pts)[None], None if c is None else _dev(env, c)[None], radius, S, blend)
                assert np.array_equal(_bits(img[0]), _bits(want))
                # the planes returned are the planes the image was made from
                back = RP.image(planes[0].cpu().numpy(), blend, np.float32).reshape(S, S, 3)
                assert np.array_equal(back.view(np.uint32), _bits(img[0]))
        # the thread's mode is what it was, and the other blend's call does not depend on it
        other, _ = P.render_points_forward(_dev(env, pts)[None], _dev(env, col)[None], 0.02, 96, 1 - blend)
        assert P.render_tune(blend) == blend
        P.render_tune(1 - blend)
        want = P.splat_image(_dev(env, pts), 0.02, 96, _dev(env, col))
        assert np.array_equal(_bits(other[0]), _bits(want))
        P.render_tune(blend)
        # three different clouds of equal size in one call
        clouds = [_cloud(10 + e, 700, 0.5 + 0.3 * e) for e in range(3)]
        bp = torch.stack([_dev(env, p) for p, _ in clouds])
        bc = torch.stack([_dev(env, c) for _, c in clouds])
        img3, pl3 = P.render_points_forward(bp, bc, 0.03, 96, blend)
        for e in range(3):
            one, pl1 = P.render_points_forward(bp[e:e + 1].contiguous(), bc[e:e + 1].contiguous(), 0.03, 96, blend)
            assert np.array_equal(_bits(img3[e]), _bits(one[0])) and np.array_equal(_bits(pl3[e]), _bits(pl1[0]))
            assert np.array_equal(_bits(img3[e]), _bits(P.splat_image(bp[e], 0.03, 96, bc[e])))
        # no points: the background
        img0, _ = P.render_points_forward(torch.empty(2, 0, 3, device="cuda"), None, 0.03, 40, blend)
        assert not img0.cpu().numpy().any()
    finally:
        P.render_tune(prev)


# ------------------------------------------------------------------------------------------------ 7. backward against float64

@pytest.mark.parametrize("name", [c["name"] for c in C.cases()])
def test_backward_against_the_float64_restatement(env, name):
    """every G kind under both blends: position and colour, per point and summed over the cloud, within MARGIN x the yardstick of
    the class (measured on the CPU: render_points_cases.YARDSTICK)"""
    case = next(c for c in C.cases() if c["name"] == name)
    S, rad = case["S"], case["radius"]
    for blend in (0, 1):
        for kind, G in C.upstream(case).items():
            want = C.reference(case, blend, kind)
            img, planes, gp, gc = _run(env, case["pts"], case["col"], rad, S, blend, G)
            gp, gc = gp[0].cpu().numpy(), gc[0].cpu().numpy()
            assert np.isfinite(gp).all() and np.isfinite(gc).all()
            e, b = C.errors(gp, gc, want), C.bars(blend, kind)
            print("%s blend %d %-10s errors %s bars %s" % (name, blend, kind, " ".join("%.2e" % x for x in e), " ".join("%.2e" % x for x in b)))
            for got, bar, what in zip(e, b, ("position of one point", "position of the cloud", "colour of one point", "colour of the cloud")):
                assert got <= bar, (name, blend, kind, what, got, bar)


# ------------------------------------------------------------------------------------------------ 8. exact zeros

@pytest.mark.parametrize("blend", (1, 0))
def test_exact_zeros(env, blend):
    for case in C.cases():
        if case["name"] not in ("posed-coloured-33", "small-radius-16", "white-deep-16", "identity-33"):
            continue
        S, rad, kinds = case["S"], case["radius"], C.upstream(case)
        seen = RP.seen(case["pts"], rad, S)
        img, planes, gp, gc = _run(env, case["pts"], case["col"], rad, S, blend, kinds["zero"])
        assert not _bits(gp).any() and not _bits(gc).any()                  # all +0: no bit set, the sign bit included
        if "hot_empty" in kinds:
            _, _, gp, gc = _run(env, case["pts"], case["col"], rad, S, blend, kinds["hot_empty"])
            assert not _bits(gp).any() and not _bits(gc).any()
        img, planes, gp, gc = _run(env, case["pts"], case["col"], rad, S, blend, kinds["dense"])
        assert (~seen).sum() >= 2 and not _bits(gp[0])[~seen].any() and not _bits(gc[0])[~seen].any()
        assert np.abs(gp[0].cpu().numpy()[seen]).max() > 0
        # without the points the camera does not see (NaN and inf among them) the others' rows are the same bits
        keep = np.flatnonzero(seen)
        col = None if case["col"] is None else case["col"][keep]
        img2, planes2, gp2, gc2 = _run(env, case["pts"][keep], col, rad, S, blend, kinds["dense"])
        assert np.array_equal(_bits(img2), _bits(img)) and np.array_equal(_bits(planes2), _bits(planes))
        assert np.array_equal(_bits(gp2[0]), _bits(gp[0])[keep]) and np.array_equal(_bits(gc2[0]), _bits(gc[0])[keep])


# ------------------------------------------------------------------------------------------------ 9. determinism

@pytest.mark.parametrize("blend", (1, 0))
def test_backward_is_deterministic(env, blend):
    torch, P = env["torch"], env["P"]
    S, rad, n = 96, 0.03, 2451
    clouds = [_cloud(40 + e, n, 0.6 + 0.2 * e, 0.1) for e in range(3)]
    rng = np.random.default_rng(5)
    G = torch.stack([_dev(env, rng.random((S, S, 3)) - 0.5) for _ in range(3)])
    bp = torch.stack([_dev(env, p) for p, _ in clouds])
    bc = torch.stack([_dev(env, c) for _, c in clouds])
    img, planes = P.render_points_forward(bp, bc, rad, S, blend)
    gp, gc = P.render_points_backward(bp, bc, rad, S, blend, planes, G)
    assert np.abs(gp.cpu().numpy()).max() > 0 and np.abs(gc.cpu().numpy()).max() > 0
    gp2, gc2 = P.render_points_backward(bp, bc, rad, S, blend, planes, G)
    assert np.array_equal(_bits(gp), _bits(gp2)) and np.array_equal(_bits(gc), _bits(gc2))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        img3, planes3 = P.render_points_forward(bp, bc, rad, S, blend)
        gp3, gc3 = P.render_points_backward(bp, bc, rad, S, blend, planes3, G)
    side.synchronize()
    assert np.array_equal(_bits(planes3), _bits(planes)) and np.array_equal(_bits(gp), _bits(gp3)) and np.array_equal(_bits(gc), _bits(gc3))
    for e in range(3):
        p1, c1 = bp[e:e + 1].contiguous(), bc[e:e + 1].contiguous()
        _, pl1 = P.render_points_forward(p1, c1, rad, S, blend)
        g1, k1 = P.render_points_backward(p1, c1, rad, S, blend, pl1, G[e:e + 1].contiguous())
        assert np.array_equal(_bits(g1[0]), _bits(gp[e])) and np.array_equal(_bits(k1[0]), _bits(gc[e]))
    gp4, none = P.render_points_backward(bp, bc, rad, S, blend, planes, G, want_col=False)
    assert none is None and np.array_equal(_bits(gp4), _bits(gp))
    # white (col == NULL): the colour gradient may still be asked for
    _, plw = P.render_points_forward(bp, None, rad, S, blend)
    gw, kw = P.render_points_backward(bp, None, rad, S, blend, plw, G)
    ones = torch.ones_like(bp)
    _, plo = P.render_points_forward(bp, ones, rad, S, blend)
    go, ko = P.render_points_backward(bp, ones, rad, S, blend, plo, G)
    assert np.array_equal(_bits(gw), _bits(go)) and np.array_equal(_bits(kw), _bits(ko))


# ------------------------------------------------------------------------------------------------ 10. autograd

def test_autograd_layer(env):
    torch, P = env["torch"], env["P"]
    S, rad = 64, 0.04
    pts, col = _cloud(7, 500, 0.7, 0.1)
    G = _dev(env, np.random.default_rng(3).random((S, S, 3)) - 0.5)
    prev = P.render_tune(-1)
    try:
        for blend in (1, 0):
            p, c = _dev(env, pts).requires_grad_(True), _dev(env, col).requires_grad_(True)
            img = P.render_points(p, c, rad, S, blend=blend)
            assert img.shape == (S, S, 3)
            (img * G).sum().backward()
            _, planes = P.render_points_forward(p.detach()[None], c.detach()[None], rad, S, blend)
            gp, gc = P.render_points_backward(p.detach()[None], c.detach()[None], rad, S, blend, planes, G[None])
            assert np.array_equal(_bits(p.grad), _bits(gp[0])) and np.array_equal(_bits(c.grad), _bits(gc[0]))
            # blend=None: the thread's mode at forward time, whatever is set by the time of the backward
            P.render_tune(blend)
            p2 = _dev(env, pts).requires_grad_(True)
            img2 = P.render_points(p2, _dev(env, col), rad, S)
            assert np.array_equal(_bits(img2), _bits(img))
            P.render_tune(1 - blend)
            (img2 * G).sum().backward()
            assert np.array_equal(_bits(p2.grad), _bits(gp[0]))
            P.render_tune(-1)
            # colours that do not require grad get none; no colours at all; a batch
            c3 = _dev(env, col)
            p3 = _dev(env, pts).requires_grad_(True)
            (P.render_points(p3, c3, rad, S, blend=blend) * G).sum().backward()
            assert c3.grad is None and np.array_equal(_bits(p3.grad), _bits(gp[0]))
            p4 = _dev(env, pts).requires_grad_(True)
            (P.render_points(p4, None, rad, S, blend=blend) * G).sum().backward()
            assert p4.grad is not None and torch.isfinite(p4.grad).all()
            p5 = torch.stack([_dev(env, pts), _dev(env, pts[::-1].copy())]).requires_grad_(True)
            img5 = P.render_points(p5, None, rad, S, blend=blend)
            assert img5.shape == (2, S, S, 3)
            (img5[0] * G).sum().backward()
            assert np.array_equal(_bits(p5.grad[0]), _bits(p4.grad)) and not _bits(p5.grad[1]).any()
        with pytest.raises(RuntimeError, match="GPU tensors only"):
            P.render_points(torch.zeros(4, 3))
        with pytest.raises(ValueError):
            P.render_points(_dev(env, pts), _dev(env, col[:10]), rad, S)
    finally:
        P.render_tune(prev)


# ------------------------------------------------------------------------------------------------ 11. refusals

def test_refusals_touch_nothing(env):
    """-1 with the error recorded and nothing enqueued: every buffer here is 64 floats, far shorter than the arguments claim, with a
    pattern that must still stand; n == 0 returns 1"""
    torch, lib = env["torch"], env["lib"]
    L, p = lib.lib, lib.ptr
    names = ("pts", "col", "img", "planes", "grad_img", "grad_pts", "grad_col")
    buf = {k: torch.full((64,), 7.25, device="cuda") for k in names}
    st = lib.stream_of(buf["pts"])

    def fwd(b=2, n=100000, radius=0.02, size=224, blend=1, pts="pts", img="img"):
        return L.genpc_render_points(b, n, p(buf.get(pts)), p(buf["col"]), radius, size, blend, p(buf.get(img)), p(buf["planes"]), st)

    def bwd(b=2, n=100000, radius=0.02, size=224, blend=1, pts="pts", planes="planes", grad_img="grad_img", grad_pts="grad_pts"):
        return L.genpc_render_points_backward(b, n, p(buf.get(pts)), p(buf["col"]), radius, size, blend, p(buf.get(planes)), p(buf.get(grad_img)),
                                              p(buf.get(grad_pts)), p(buf["grad_col"]), st)
    bad = [dict(b=0), dict(b=-1), dict(n=-1), dict(size=0), dict(size=-3), dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")),
           dict(blend=2), dict(blend=-1), dict(pts=None)]
    for kw in bad + [dict(img=None)]:
        assert fwd(**kw) == -1, kw
        assert b"genpc_render_points" in L.genpc_last_error()
    for kw in bad + [dict(planes=None), dict(grad_img=None), dict(grad_pts=None)]:
        assert bwd(**kw) == -1, kw
        assert b"genpc_render_points_backward" in L.genpc_last_error()
    assert bwd(n=0, pts=None, planes=None, grad_img=None, grad_pts=None) == 1      # nothing to do, nothing written
    torch.cuda.synchronize()
    for k in names:
        assert bool((buf[k] == 7.25).all()), k


# ------------------------------------------------------------------------------------------------ 12. the composed objective

@pytest.mark.parametrize("blend", (1, 0))
def test_composed_objective_against_the_oracle(env, oracle, blend):
    """The pose in torch, render_points, compute_loss_function with chamfer_3DDist's autograd, the orthogonality term: loss terms
    and the 10-vector gradient against oracle.pose_full_loss_grad at test_gpu_geometry.py's bars (the inputs and the assertions:
    render_points_cases.objective_*; tests/test_render_points_cases.py holds the same composition to them on the CPU)."""
    torch, P = env["torch"], env["P"]
    from genpc_amd.utils.loss_util import Completionloss
    cdloss = Completionloss(loss_func="cd_l1")
    o = {k: _dev(env, v) for k, v in C.objective_inputs().items()}
    o["chamfer"] = lambda pts, partial: (cdloss.chamfer_partial_l1(pts[None], partial[None]), cdloss.chamfer_partial_l1(partial[None], pts[None]))
    render = lambda pts, col, radius, size: P.render_points(pts, col, radius, size, blend=blend)
    for radius, size in C.OBJECTIVE_CONFIGS:
        want = C.objective_reference(oracle, blend, radius, size)
        with torch.no_grad():
            ref = P.render_points(o["partial"], o["pcol"], radius, size, blend=blend)
        loss4, grad = C.torch_objective(P, render, o, dict(want, ref_img_t=ref), radius, size)
        print("blend %d size %d loss %s oracle %s" % (blend, size, loss4, want["loss"]))
        print("grad %s\noracle %s" % (grad, want["grad"]))
        C.objective_check(loss4, grad, want)


# ------------------------------------------------------------------------------------------------ 13. the torch loop

@pytest.mark.parametrize("blend", (1, 0))
def test_torch_loop_against_the_oracle(env, oracle, blend):
    """object_pose_optimization_torch's first steps track oracle.pose_optimize's at the bar test_pose_loop_full_objective holds the
    fused loop to (rtol 5e-3), and a changed objective -- weights with an edge term -- moves the history by more than that bar;
    a loss_fn that adds 0.5 mse (0.3 % of this loss) raises every start's first entry and moves the rest."""
    torch, P = env["torch"], env["P"]
    complete, partial = C.shape(9, 1200)
    rng = np.random.default_rng(12)
    ccol, pcol = C.colours(rng, len(complete), 0.25), C.colours(rng, len(partial))
    Cd, Pd, cc, pc = (_dev(env, x) for x in (complete, partial, ccol, pcol))
    kw = dict(radius=0.02, lr=0.01, iters=10, render_size=224, cam_bias_num=4, complete_col=cc, partial_col=pc, return_history=True)
    prev_l, prev_o = P.render_tune(blend), oracle.set_blend(blend)
    try:
        T, hist, bp = P.object_pose_optimization_torch(Cd, Pd, **kw)
        oT, ohist, obp = oracle.pose_optimize(complete, partial, lr=0.01, iters=10, starts=4, radius=0.02, size=224, complete_col=ccol,
                                              partial_col=pcol)
        print("history\n%s\noracle\n%s" % (hist[:, :10], ohist[:, :10]))
        assert hist.shape == (4, 11) and np.isfinite(hist).all() and T.shape == (4, 4) and T[3].tolist() == [0, 0, 0, 1] and bp.shape == (10,)
        np.testing.assert_allclose(hist[:, :10], ohist[:, :10], rtol=5e-3)
        from genpc_amd.utils.loss_util import Completionloss
        cdloss = Completionloss(loss_func="cd_l1")
        eye = torch.eye(3, device="cuda")

        def with_mse(ref_img, result, ref_mask, partial_xyz, pts, R_obj):
            out = P.compute_loss_function(ref_img, result, ref_mask, partial_xyz, pts, cdloss)
            return out[0] + 0.5 * out[1] + 0.001 * torch.norm(R_obj @ R_obj.T - eye)
        _, h_mse, _ = P.object_pose_optimization_torch(Cd, Pd, loss_fn=with_mse, **kw)
        _, h_edge, _ = P.object_pose_optimization_torch(Cd, Pd, weights=dict(edge=20.0), **kw)
        print("with 0.5 mse\n%s\nwith 20 edge\n%s" % (h_mse[:, :10], h_edge[:, :10]))
        assert np.isfinite(h_mse).all() and (h_mse[:, 0] > hist[:, 0]).all() and (h_mse[:, 1:] != hist[:, 1:]).all()      # (the same pose at step 0, and mse > 0)
        assert np.isfinite(h_edge).all() and (np.abs(h_edge[:, :10] - hist[:, :10]) > 5e-3 * np.abs(hist[:, :10])).all()
        # a loss_fn that restates the default objective gives the default's history
        same = lambda ref_img, result, ref_mask, partial_xyz, pts, R_obj: \
            P.compute_loss_function(ref_img, result, ref_mask, partial_xyz, pts, cdloss)[0] + 0.001 * torch.norm(R_obj @ R_obj.T - eye)
        _, h_same, _ = P.object_pose_optimization_torch(Cd, Pd, loss_fn=same, **dict(kw, cam_bias_num=1))
        # (not bit for bit: the dense Chamfer backward under chamfer_3DDist adds with floating-point atomics, in arrival order)
        np.testing.assert_allclose(h_same[0], hist[0], rtol=1e-4)
    finally:
        P.render_tune(prev_l)
        oracle.set_blend(prev_o)
