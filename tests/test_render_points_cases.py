"""render_points' numpy restatement (tests/render_points_ref.py) and its cases (tests/render_points_cases.py) on the CPU: the
float64 restatement against finite differences of its own forward, the yardsticks the GPU tests' bars come from, the signal an
all-zero answer would miss, the torch helpers of genpc_amd.optim_registration.diff_obj_pose against the reference's own code
(tests/golden/ref_py_objective.npz), and the composed torch objective -- the numpy renderer standing in -- against the oracle
on the inputs tests/test_gpu_render_points.py uses on the device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_loss_ref as R                # noqa: E402
import render_points_cases as C          # noqa: E402
import render_points_ref as RP           # noqa: E402

# The finite differences.  A step moves no pixel's coverage a by more than FD_DA = 1e-2 A_MARGIN, so no a crosses 0 or 0.999 (the
# conditions keep every a A_MARGIN away from both).  What a central difference then leaves: a pixel's value is a ratio
# (N0 + w c) / (D0 + w) in the weight w of the moving disc, whose third derivative is 6 / (D0 + w)^2 of its first, and D0 + w >= w
# >= a >= A_MARGIN: (FD_DA / A_MARGIN)^2 = 1e-4 of the pixel's term at the worst, 2e-4 with the depth's share; rounding: 1e-16 of
# the box's L over a step of 1e-8 (`noise` below, 64 spacings of the box's sum of magnitudes).  The colour enters linearly: its difference is exact.
FD_DA = 1e-2 * C.A_MARGIN
FD_TOL = 2e-4
FD_COL_STEP = 1e-3


def _fd_steps(p, radius, S):
    """world steps (x, y, z) that move no coverage of the point's box by more than FD_DA"""
    u, v, rho, zv, ok = [x[0] for x in R.project(p, radius, S)]
    f4, hs = 0.5 * S * R.FOCAL, 0.5 * S
    reach = rho + 1.5                                          # |dx|, |dy| of the box's pixel centres
    da_du = 2.0 * reach / (rho * rho)
    da_xy = da_du * f4 / zv
    da_z = (da_du * (abs(u - hs) + abs(v - hs)) + 2.0 * reach * reach * 2.0 / (rho * rho)) / zv
    return FD_DA / da_xy, FD_DA / da_xy, FD_DA / da_z


def _neighbours(pts, i, radius, S):
    """the points whose disc's box meets point i's (the others do not touch the pixels point i can change), and that box as a mask"""
    ok = RP.seen(pts, radius, S)
    u, v, rho, zv, _ = R.project(RP.drawable(pts), radius, S)
    near = ok & (np.abs(u - u[i]) <= rho + rho[i] + 3) & (np.abs(v - v[i]) <= rho + rho[i] + 3)
    c0, c1, r0, r1 = R.box(float(u[i]), float(v[i]), float(rho[i]) + 1.0, S)
    mask = np.zeros((S, S), bool)
    mask[r0:r1 + 1, c0:c1 + 1] = True
    idx = np.flatnonzero(near)
    return idx, int(np.flatnonzero(idx == i)[0]), mask.reshape(-1)


def _tested_points(case):
    seen = RP.seen(case["pts"], case["radius"], case["S"])
    generic = lambda n: n[:2] in ("bg", "co", "mi") or (n[0] in "pw" and n[1:].isdigit())
    named = [i for i, n in enumerate(case["names"]) if seen[i] and not generic(n)]
    others = [i for i, n in enumerate(case["names"]) if seen[i] and generic(n)][:10]
    return named + others


def test_cases_stand():
    names = [c["name"] for c in C.cases()]
    assert len(set(names)) == len(names) and {c["S"] for c in C.cases()} == {16, 33}
    sizes = [len(c["pts"]) for c in C.cases()]
    assert min(sizes) >= 5 and max(sizes) >= 300
    wanted = {"left", "right", "top", "bottom", "corner", "outside", "behind_eye", "at_zfar", "past_zfar", "on_centre", "tiny", "huge",
              "tall", "nan", "inf"}
    assert wanted <= {n for c in C.cases() for n in c["names"]}
    assert any(c["col"] is None for c in C.cases())
    for case in C.cases():
        assert not C.conditions(case), (case["name"], C.conditions(case))
        seen = RP.seen(case["pts"], case["radius"], case["S"])
        for n in ("nan", "inf", "behind_eye", "past_zfar"):
            if n in case["names"]:
                assert not seen[case["names"].index(n)]
        kinds = C.upstream(case)
        assert {"dense", "zero"} <= set(kinds)
    assert all(any(k in C.upstream(c) for c in C.cases()) for k in ("hot_inside", "hot_rim", "hot_empty"))


def test_rows_form_of_the_forward_is_the_dense_one():
    case = next(c for c in C.cases() if c["name"] == "together-33-33")
    for blend in (0, 1):
        a = R.planes_of(RP.drawable(case["pts"]), case["col"], case["radius"], case["S"], blend)
        b = RP.planes_by_rows(RP.drawable(case["pts"]), case["col"], case["radius"], case["S"], blend, rows=5)
        np.testing.assert_allclose(b, a, rtol=1e-13, atol=0)
        assert np.array_equal(b[0], a[0])


@pytest.mark.parametrize("blend", (0, 1))
def test_float64_restatement_against_finite_differences(blend):
    """d L / d xyz and d L / d colour of L = sum G . I for every named seen point and ten others of every case"""
    worst = 0.0
    for case in C.cases():
        S, rad = case["S"], case["radius"]
        G = C.upstream(case)["dense"].astype(np.float64).reshape(-1, 3)
        want = C.reference(case, blend, "dense")
        col_all = np.ones((len(case["pts"]), 3)) if case["col"] is None else case["col"].astype(np.float64)
        for i in _tested_points(case):
            idx, me, mask = _neighbours(case["pts"], i, rad, S)
            sub, subcol = case["pts"][idx].astype(np.float64), col_all[idx]

            def L(p=None, c=None):
                pp, cc = sub.copy(), subcol.copy()
                if p is not None:
                    pp[me] = p
                if c is not None:
                    cc[me] = c
                img = RP.image(R.planes_of(pp, cc, rad, S, blend), blend)
                return float((G[mask] * img[mask]).sum())
            steps = _fd_steps(sub[me], rad, S)
            base = RP.image(R.planes_of(sub, subcol, rad, S, blend), blend)
            noise = 64 * 2.0 ** -52 * float(np.abs(G[mask] * base[mask]).sum())      # what rounding leaves of a difference of two L
            for k in range(3):
                d = np.zeros(3)
                d[k] = steps[k]
                fd = (L(p=sub[me] + d) - L(p=sub[me] - d)) / (2 * steps[k])
                err = abs(fd - want["gp"][i, k])
                assert err <= FD_TOL * want["sp"][i, k] + noise / steps[k], (case["name"], case["names"][i], "xyz"[k], fd, want["gp"][i, k], want["sp"][i, k])
                if FD_TOL * want["sp"][i, k] > noise / steps[k]:      # (a sum hidden behind a nearer disc is below the rounding of L)
                    worst = max(worst, err / want["sp"][i, k])
            for k in range(3):
                d = np.zeros(3)
                d[k] = FD_COL_STEP
                fd = (L(c=subcol[me] + d) - L(c=subcol[me] - d)) / (2 * FD_COL_STEP)
                assert abs(fd - want["gc"][i, k]) <= 1e-9 * want["sc"][i, k] + noise / FD_COL_STEP, (case["name"], case["names"][i], "rgb"[k], fd, want["gc"][i, k])
    print("blend %d: worst finite-difference error %.3g of a sum's magnitude" % (blend, worst))


def test_unseen_and_non_finite_points_have_zero_rows():
    for case in C.cases():
        for blend in (0, 1):
            want = C.reference(case, blend, "dense")
            off = ~want["seen"]
            assert off.sum() >= 2 and not want["gp"][off].any() and not want["gc"][off].any() and not want["sp"][off].any()
            zero = C.reference(case, blend, "zero")
            assert not zero["gp"].any() and not zero["gc"].any()
            if "hot_empty" in C.upstream(case):
                e = C.reference(case, blend, "hot_empty")
                assert not e["gp"].any() and not e["gc"].any()


def test_yardsticks_are_the_recorded_ones():
    """float32 restatement against float64, per class: not above the recorded value, not below a third of it"""
    got = C.measure()
    assert set(got) == set(C.YARDSTICK)
    for k, vals in got.items():
        for g, rec in zip(vals, C.YARDSTICK[k]):
            assert rec / 3 <= g <= rec, (k, vals, C.YARDSTICK[k])


def test_an_all_zero_answer_would_be_seen():
    for case in C.cases():
        for blend in (0, 1):
            col, pos = C.signal(C.reference(case, blend, "dense"))
            b = C.bars(blend, "dense")
            assert col >= 10 * b[2], (case["name"], blend, col, b[2])
            assert pos >= 100 * b[1], (case["name"], blend, pos, b[1])


# ------------------------------------------------------------------------------------------------ the torch helpers

def test_torch_helpers_match_the_reference_code(golden):
    """edge_loss, soft_iou_loss, dice_loss, compute_soft_mask, normalize_images and compute_loss_function against the reference's own
    code in float32 (tests/golden/make_reference_objective_vectors.py), at test_reference_vectors.py's tolerances for the mask loss:
    values 1e-4 relative, the gradient 2e-3 of its largest entry at the worst and 1e-4 on average."""
    import torch
    from genpc_amd.optim_registration import diff_obj_pose as P
    g = golden("ref_py_objective.npz")
    close = lambda a, b: np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=1e-4, atol=1e-6)
    for name in g["cases"]:
        ref, res, rmask = (torch.from_numpy(g[name + k]) for k in ("_ref", "_result", "_refmask"))
        assert np.array_equal(P.compute_mask_from_rendering(ref).numpy(), g[name + "_refmask"])
        close(P.edge_loss(ref, res), g[name + "_edge"])
        l, v, soft = P.soft_iou_loss(res, rmask)
        close([l, v], g[name + "_iou"])
        close(soft, g[name + "_iou_soft"])
        close(P.compute_soft_mask(res), g[name + "_softmask"])
        close(P.dice_loss(P.compute_soft_mask(res), P.compute_soft_mask(ref)), g[name + "_dice"])
        close(P.normalize_images(ref, res)[1], g[name + "_norm_statistical"])
        close(P.normalize_images(ref, res, method="histogram")[1], g[name + "_norm_histogram"])
        assert P.normalize_images(ref, res, method="none")[1] is res
        q = res.clone().requires_grad_(True)
        out = P.compute_loss_function(ref, q, rmask)
        assert len(out) == 7
        close([float(x) for x in out], g[name + "_tuple"])
        out[0].backward()
        wgrad = g[name + "_grad"]
        scale = np.abs(wgrad).max()
        assert np.abs(q.grad.numpy() - wgrad).max() <= 2e-3 * scale and np.abs(q.grad.numpy() - wgrad).mean() <= 1e-4 * scale
        # the weights: the default is the reference's; a term turned on enters the total with its weight
        mse, edge, iou = float(out[1]), float(P.edge_loss(*P.normalize_images(ref, res))), float(out[3])
        w = P.compute_loss_function(ref, res, rmask, weights=dict(mse=2.0, edge=0.5, iou=0.25))
        close(float(w[0]), float(out[0]) + 2.0 * mse + 0.5 * edge + 0.25 * iou)
        close(float(w[2]), edge)
        close(float(P.compute_loss_function(ref, res, rmask, weights=(0, 0, 1, 0, 3))[0]), float(out[0]))
    with pytest.raises(ValueError):
        P.compute_loss_function(ref, res, weights=dict(colour=1.0))


def test_rotation_helpers():
    import math
    import torch
    from genpc_amd.optim_registration import diff_obj_pose as P
    for k in range(4):
        th = math.radians(90.0 * k)
        r6 = P.get_init_rot("y", 90 * k, "cpu")
        np.testing.assert_allclose(r6.numpy(), np.float32([math.cos(th), 0, math.sin(th), 0, 1, 0]), atol=1e-7)
        Rm = P.rotation_6d_to_matrix(r6[None])[0].numpy()
        np.testing.assert_allclose(Rm, [[math.cos(th), 0, math.sin(th)], [0, 1, 0], [-math.sin(th), 0, math.cos(th)]], atol=1e-6)
    d6 = torch.tensor([0.9, 0.1, -0.3, 0.05, 1.1, 0.2])
    np.testing.assert_allclose(P.rotation_6d_to_matrix(d6).numpy(), R.rot6d(d6.numpy()), atol=1e-6)
    axis = P.get_init_rot([0.0, 0.0, 2.0], 90, "cpu")
    np.testing.assert_allclose(axis.numpy(), [0, -1, 0, 1, 0, 0], atol=1e-6)
    with pytest.raises(ValueError):
        P.get_init_rot("w", 10, "cpu")
    T = P.build_transform(torch.eye(3), torch.tensor([0.1, -0.2, 0.3]), torch.tensor(0.8)).numpy()
    np.testing.assert_allclose(T, [[0.8, 0, 0, 0.1], [0, 0.8, 0, -0.2], [0, 0, 0.8, 0.3], [0, 0, 0, 1]], atol=1e-7)


def test_cpu_tensors_and_other_cameras_are_refused():
    import torch
    from genpc_amd.optim_registration import diff_obj_pose as P
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        P.render_points(torch.zeros(4, 3))
    with pytest.raises(ValueError, match="one camera"):
        P.ObjectPoseOptim(torch.zeros(4, 3), None, 0.02, 32, "cpu", torch.eye(3)[None], torch.tensor([[0.0, 0.0, 3.0]]), P.get_init_rot("y", 0, "cpu"))
    Rc = torch.tensor([[[-1.0, 0, 0], [0, 1, 0], [0, 0, -1]]])
    with pytest.raises(ValueError, match="focal"):
        P.ObjectPoseOptim(torch.zeros(4, 3), None, 0.02, 32, "cpu", Rc, torch.tensor([[0.0, 0.0, 3.0]]), P.get_init_rot("y", 0, "cpu"), focal=2.0)
    m = P.ObjectPoseOptim(torch.rand(4, 3), None, 0.02, 32, "cpu", Rc, torch.tensor([[0.0, 0.0, 3.0]]), P.get_init_rot("y", 90, "cpu"))
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == ["log_scale", "rot_6d", "trans"]
    assert abs(float(m.log_scale) - np.log(0.75)) < 1e-7 and m.get_transform().shape == (4, 4)


# ------------------------------------------------------------------------------------------------ the composed objective

@pytest.mark.parametrize("blend", (1, 0))
def test_torch_objective_with_the_numpy_renderer_against_the_oracle(oracle, blend):
    """What tests/test_gpu_render_points.py's composed-objective test relies on, without the device: with render_points_ref standing
    in for the renderer (forward and backward in float64 on the float32 posed points), the float32 torch objective's loss terms
    and 10-vector gradient lie within that test's bars of oracle.pose_full_loss_grad on that test's inputs."""
    import torch
    from genpc_amd.optim_registration import diff_obj_pose as P

    class NumpyRender(torch.autograd.Function):
        @staticmethod
        def forward(ctx, pts, col, radius, size):
            p, c = pts.detach().numpy(), col.numpy()
            pl = RP.planes(p, c, radius, size, blend)
            ctx.saved = (p, c, radius, size, pl)
            return torch.from_numpy(RP.image(pl, blend).reshape(size, size, 3).astype(np.float32))

        @staticmethod
        def backward(ctx, g):
            p, c, radius, size, pl = ctx.saved
            gp, _ = RP.backward(p, c, radius, size, blend, pl, g.numpy().astype(np.float64))
            return torch.from_numpy(gp.astype(np.float32)), None, None, None

    o = {k: torch.from_numpy(v) for k, v in C.objective_inputs().items()}
    for radius, size in C.OBJECTIVE_CONFIGS:
        want = C.objective_reference(oracle, blend, radius, size)
        want = dict(want, ref_img_t=torch.from_numpy(want["ref_img"]))
        i1, i2 = torch.from_numpy(want["i1"].astype(np.int64)), torch.from_numpy(want["i2"].astype(np.int64))

        def chamfer(pts, partial):      # the oracle's neighbours; the distances and their derivative are torch's
            return (torch.sqrt(((pts - partial[i1]) ** 2).sum(-1)).mean(), torch.sqrt(((partial - pts[i2]) ** 2).sum(-1)).mean())
        loss4, grad = C.torch_objective(P, NumpyRender.apply, dict(o, chamfer=chamfer), want, radius, size)
        C.objective_check(loss4, grad, want)
