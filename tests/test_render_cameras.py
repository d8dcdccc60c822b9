"""The camera pieces of render_points_ragged (genpc_amd.optim_registration.diff_obj_pose: look_at_view_transform, camera_points) on
the CPU, in float64 where values are compared: the look-at of the library's eye is the library's constants, other eyes give proper
rotations that look where they should, the library's camera maps every point onto itself bit for bit, the map commutes with a
joint turn of world and camera, the mapped points with the scaled radius project -- through the renderer's numpy restatement --
where the pinhole formulas put them, and the gradients to the points, R and T are autograd's (gradcheck) and, chained by hand
behind the numpy renderer's backward, those of a two-view loss (central differences of its forward, at
tests/test_render_points_cases.py's tolerances for that comparison)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_loss_ref as R                # noqa: E402
import render_points_cases as C          # noqa: E402
import render_points_ref as RP           # noqa: E402
from test_render_points_cases import FD_TOL, _fd_steps      # noqa: E402

from genpc_amd.optim_registration import diff_obj_pose as P      # noqa: E402

EYES = [(0.0, 0.0, 3.0), (1.2, 0.6, 2.6), (-2.0, 0.3, 1.5), (0.4, -1.7, -2.2), (3.0, 0.0, 0.0)]


def test_look_at_of_the_library_eye_is_the_library_camera():
    Rc, Tc = P.look_at_view_transform((0.0, 0.0, 3.0))
    assert Rc.dtype == torch.float32 and tuple(Rc.shape) == (1, 3, 3) and tuple(Tc.shape) == (1, 3)
    assert torch.equal(Rc, torch.tensor([P._CAMERA_R])) and torch.equal(Tc, torch.tensor([P._CAMERA_T]))
    assert not torch.signbit(Rc).logical_and(Rc == 0).any() and not torch.signbit(Tc).logical_and(Tc == 0).any()      # no negative zeros
    # ... and what render_reference_image returns today
    assert Rc.tolist() == [[[-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]]] and Tc.tolist() == [[0.0, 0.0, 3.0]]
    with pytest.raises(ValueError, match="parallel"):
        P.look_at_view_transform((0.0, 2.0, 0.0))


def test_look_at_of_other_eyes():
    at = (0.1, -0.2, 0.05)
    Rc, Tc = P.look_at_view_transform(EYES, at=at)
    assert tuple(Rc.shape) == (len(EYES), 3, 3) and tuple(Tc.shape) == (len(EYES), 3)
    Rd, Td = Rc.double(), Tc.double()
    for k, eye in enumerate(EYES):
        np.testing.assert_allclose((Rd[k].T @ Rd[k]).numpy(), np.eye(3), atol=1e-6)          # (float32 entries)
        assert abs(float(torch.linalg.det(Rd[k])) - 1.0) < 1e-6
        np.testing.assert_allclose((-Td[k] @ Rd[k].T).numpy(), eye, atol=1e-6)
        # the look-at point lies on the optical axis, in front: it projects to the image centre
        xv = torch.tensor(at, dtype=torch.float64) @ Rd[k] + Td[k]
        assert abs(float(xv[0])) < 1e-6 and abs(float(xv[1])) < 1e-6 and float(xv[2]) > 0
        p = P.camera_points(torch.tensor([at], dtype=torch.float64), Rd[k], Td[k], 4.0).numpy()
        u, v, rho, zv, ok = R.project(p, 0.01, 32)
        assert ok[0] and abs(u[0] - 16.0) < 1e-4 and abs(v[0] - 16.0) < 1e-4
    # up is +y: a point above the look-at point is drawn above the centre (a smaller row)
    Rk, Tk = P.look_at_view_transform((1.2, 0.6, 2.6))
    p = P.camera_points(torch.tensor([[0.0, 0.2, 0.0]], dtype=torch.float64), Rk[0], Tk[0], 4.0).numpy()
    assert R.project(p, 0.01, 32)[1][0] < 16.0


@pytest.mark.parametrize("dtype", (torch.float32, torch.float64))
def test_the_library_camera_is_the_identity_bit_for_bit(dtype):
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(4000, 3, generator=g, dtype=torch.float64) * 4 - 2).to(dtype)
    x[:6] = torch.tensor([[1e-30, -1e30, 3.0], [0.0, 0.0, 0.0], [1.5, -0.25, 2.999999], [float("inf"), 1.0, 2.0], [float("nan"), 0.0, 0.0],
                          [7.0, 8.0, 9.0]], dtype=dtype)
    y = P.camera_points(x, torch.tensor(P._CAMERA_R), torch.tensor(P._CAMERA_T), 4.0)
    assert y.dtype == dtype
    fin = torch.isfinite(x).all(dim=1)
    assert torch.equal(y[fin], x[fin]) and not torch.isfinite(y[~fin]).all(dim=1).any()
    view = torch.int32 if dtype == torch.float32 else torch.int64
    assert torch.equal(y[fin].view(view), x[fin].view(view))
    # the look-at's own output, and the batched forms of R and T a list call takes
    Rc, Tc = P.look_at_view_transform((0.0, 0.0, 3.0))
    assert torch.equal(P.camera_points(x[fin], Rc[0], Tc[0], 4.0).view(view), x[fin].view(view))


def test_signed_permutations_and_power_of_two_focals_map_without_rounding():
    g = torch.Generator().manual_seed(6)
    x = torch.rand(500, 3, generator=g) * 2 - 1
    Rp = torch.tensor([[0.0, 0.0, -1.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])      # X_view = (-y, z, -x)
    for f in (2.0, 4.0, 8.0):
        y = P.camera_points(x, Rp, torch.tensor([0.0, 0.0, 3.0]), f)
        xv = np.stack([-x[:, 1].numpy(), x[:, 2].numpy(), -x[:, 0].numpy()], axis=1)
        want = np.stack([np.float32(-f / 4) * xv[:, 0], np.float32(f / 4) * xv[:, 1], -xv[:, 2]], axis=1).astype(np.float32)
        assert np.array_equal(y.numpy(), want)


def test_a_joint_turn_of_world_and_camera_changes_nothing():
    g = torch.Generator().manual_seed(7)
    x = torch.rand(300, 3, generator=g, dtype=torch.float64) * 2 - 1
    Q = torch.linalg.qr(torch.rand(3, 3, generator=g, dtype=torch.float64))[0]
    for eye, f in zip(EYES, (4.0, 3.0, 5.5, 2.0, 4.0)):
        Rc, Tc = P.look_at_view_transform(eye)
        Rd, Td = Rc[0].double(), Tc[0].double()
        a = P.camera_points(x, Rd, Td, f)
        b = P.camera_points(x @ Q, Q.T @ Rd, Td, f)
        assert float((a - b).abs().max()) <= 1e-12


def test_mapped_points_project_where_the_pinhole_formulas_put_them():
    g = torch.Generator().manual_seed(8)
    x = torch.rand(400, 3, generator=g, dtype=torch.float64) - 0.5
    S, r = 32, 0.013
    hs = 0.5 * S
    for eye, f in zip(EYES, (4.0, 3.0, 5.5, 2.0, 8.0)):
        Rc, Tc = P.look_at_view_transform(eye)
        Rd, Td = Rc[0].double(), Tc[0].double()
        xv = (x @ Rd + Td).numpy()
        p = P.camera_points(x, Rd, Td, f).numpy()
        u, v, rho, zv, ok = R.project(p, r * f / 4.0, S)
        assert RP.seen(p, r * f / 4.0, S).all() and ok.all()
        np.testing.assert_allclose(zv, xv[:, 2], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(u, hs * (1 - f * xv[:, 0] / xv[:, 2]), rtol=1e-12, atol=1e-11)
        np.testing.assert_allclose(v, hs * (1 - f * xv[:, 1] / xv[:, 2]), rtol=1e-12, atol=1e-11)
        np.testing.assert_allclose(rho, hs * f * r / xv[:, 2], rtol=1e-12, atol=0)


def test_gradcheck_of_camera_points():
    g = torch.Generator().manual_seed(9)
    x = (torch.rand(7, 3, generator=g, dtype=torch.float64) - 0.5).requires_grad_()
    Rc, Tc = P.look_at_view_transform((1.2, 0.6, 2.6))
    Rd = (Rc[0].double() + 0.01 * torch.rand(3, 3, generator=g, dtype=torch.float64)).requires_grad_()
    Td = Tc[0].double().clone().requires_grad_()
    for f in (4.0, 2.5):
        assert torch.autograd.gradcheck(lambda a, b, c: P.camera_points(a, b, c, f), (x, Rd, Td), eps=1e-6, atol=1e-9, rtol=1e-7)


# ---- a two-view loss: d L / d T and d L / d R behind the numpy renderer's backward, chained by hand, against central differences

S2, RAD2 = 32, 0.03
VIEWS2 = (((0.0, 0.0, 3.0), 4.0), ((1.2, 0.6, 2.6), 3.0))


def _margin(p, radius):
    """the smallest distance of a pixel centre's coverage from 0 and 0.999 over the seen points [n] (inf: unseen or an empty box)"""
    out = np.full(len(p), np.inf)
    seen = RP.seen(p, radius, S2)
    u, v, rho, zv, ok = R.project(p, radius, S2)
    for i in np.flatnonzero(seen):
        a = R.coverage(u[i], v[i], rho[i], S2)[5]
        if a.size:
            out[i] = min(np.abs(a).min(), np.abs(a - R.AMAX).min())
    return out


@pytest.fixture(scope="module")
def two_views():
    """At most 200 points that both cameras see with every coverage A_MARGIN from 0 and 0.999 (the finite differences' condition, as
    tests/render_points_cases.py settles its points), their colours, the cameras in float64 and an upstream gradient per view."""
    rng = np.random.default_rng(11)
    cand = rng.uniform(-0.35, 0.35, (600, 3))
    cams = []
    for eye, f in VIEWS2:
        Rc, Tc = P.look_at_view_transform(eye)
        cams.append((Rc[0].double().numpy(), Tc[0].double().numpy(), f))
    keep = np.ones(len(cand), bool)
    for Rv, Tv, f in cams:
        p = P.camera_points(torch.from_numpy(cand), torch.from_numpy(Rv), torch.from_numpy(Tv), f).numpy()
        m = _margin(p, RAD2 * f / 4.0)
        keep &= np.isfinite(m) & (m >= C.A_MARGIN)
    X = cand[keep][:120]
    assert 60 <= len(X) <= 200
    col = rng.uniform(0.1, 1.0, (len(X), 3))
    G = [rng.normal(size=(S2 * S2, 3)) for _ in cams]
    return X, col, cams, G


def _mapped(X, Rv, Tv, f):
    return P.camera_points(torch.from_numpy(X), torch.from_numpy(np.ascontiguousarray(Rv)), torch.from_numpy(np.ascontiguousarray(Tv)), f).numpy()


def _view_loss(X, col, cam, G, blend):
    Rv, Tv, f = cam
    img = RP.image(R.planes_of(_mapped(X, Rv, Tv, f), col, RAD2 * f / 4.0, S2, blend), blend)
    return float((G * img).sum()), float(np.abs(G * img).sum())


@pytest.mark.parametrize("blend", (0, 1))
def test_two_view_gradients_to_T_and_R_against_central_differences(two_views, blend):
    X, col, cams, G = two_views
    worst = 0.0
    for k, (Rv, Tv, f) in enumerate(cams):
        rad = RAD2 * f / 4.0
        d = np.array([-f / 4.0, f / 4.0, -1.0])
        p = _mapped(X, Rv, Tv, f)
        pl = R.planes_of(p, col, rad, S2, blend)
        gp, _ = RP.backward(p, col, rad, S2, blend, pl, G[k])
        sp, _ = RP.backward(p, col, rad, S2, blend, pl, G[k], absolute=True)
        # the chain by hand: p = X (R D) + (T D + c)
        gT, gR = (gp * d).sum(axis=0), X.T @ (gp * d)
        sT, sR = (sp * np.abs(d)).sum(axis=0), np.abs(X).T @ (sp * np.abs(d))
        # ... is autograd's through camera_points
        xt, rt, tt = torch.from_numpy(X), torch.from_numpy(np.ascontiguousarray(Rv)).requires_grad_(), torch.from_numpy(np.ascontiguousarray(Tv)).requires_grad_()
        P.camera_points(xt, rt, tt, f).backward(torch.from_numpy(gp))
        np.testing.assert_allclose(tt.grad.numpy(), gT, rtol=1e-12, atol=1e-12 * np.abs(gT).max())
        np.testing.assert_allclose(rt.grad.numpy(), gR, rtol=1e-12, atol=1e-12 * np.abs(gR).max())
        # the other view's image does not move with this view's camera: the two-view loss's difference is this view's
        base, mag = _view_loss(X, col, cams[k], G[k], blend)
        noise = 64 * 2.0 ** -52 * mag
        steps = np.array([_fd_steps(q, rad, S2) for q in p])          # [n,3] steps in the library's frame
        for a in range(3):
            h = float((steps[:, a] / abs(d[a])).min())
            e = np.zeros(3)
            e[a] = h
            fd = (_view_loss(X, col, (Rv, Tv + e, f), G[k], blend)[0] - _view_loss(X, col, (Rv, Tv - e, f), G[k], blend)[0]) / (2 * h)
            err = abs(fd - gT[a])
            assert err <= FD_TOL * sT[a] + noise / h, ("T", k, a, fd, gT[a], sT[a])
            worst = max(worst, err / sT[a])
            for i in range(3):
                h = float((steps[:, a] / (np.abs(X[:, i]) * abs(d[a]))).min())
                E = np.zeros((3, 3))
                E[i, a] = h
                fd = (_view_loss(X, col, (Rv + E, Tv, f), G[k], blend)[0] - _view_loss(X, col, (Rv - E, Tv, f), G[k], blend)[0]) / (2 * h)
                err = abs(fd - gR[i, a])
                assert err <= FD_TOL * sR[i, a] + noise / h, ("R", k, i, a, fd, gR[i, a], sR[i, a])
                worst = max(worst, err / sR[i, a])
    assert worst > 0.0          # (a difference was taken)
    print("blend %d: worst finite-difference error %.3g of a sum's magnitude" % (blend, worst))
