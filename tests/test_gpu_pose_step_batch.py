"""One alignment step of b elements (genpc_pose_loss_grad_batch: the loop's launches at b elements, every width from
csrc/pose_plan.h) against the fp64 oracle, element by element, at the shapes of tests/pose_step_shapes.py -- the kernel forms
the plans select for wide calls: one lane per point in mask_grad_kernel, xcd_block's mapping of whole images to XCDs, pose_grad
with the 24-block cap and a second grid-stride pass (alone and riding in mask_grad's launch), pose_update_kernel on two blocks,
and every per-image kernel at blockIdx.y > 0 with exact per-element numbers.  tests/test_pose_step_shapes.py checks without a
GPU that each shape still selects its form.

Tolerances are those tests/test_gpu_geometry.py holds the single-element path to: the wide forms do the same arithmetic in
another order.  The reference of a row is computed once per renderer and colouring and shared by the tests of this file.
Each comparison prints its worst deviation / tolerance (loss, the gradient's three groups) before it asserts."""
import numpy as np
import pytest

import pose_step_shapes as shapes

pytestmark = pytest.mark.gpu

GROUPS = (slice(0, 6), slice(6, 9), slice(9, 10))
FULL_TOL = dict(l_rtol=2e-4, l_atol=1e-5, g_rel=2e-3, g_abs=1e-6)        # test_gpu_geometry.py, full objective
CD_TOL = dict(l_rtol=2e-5, l_atol=1e-6, g_rel=1e-4, g_abs=0.0)          # test_pose_transform_and_gradient


@pytest.fixture(scope="module")
def gp():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd.optim_registration import diff_obj_pose as POSE
    return dict(torch=torch, POSE=POSE)


@pytest.fixture(params=[1, 0], ids=["pulsar_blend", "coverage_splat"])
def render_blend(request, gp, oracle):
    """Both renderers of the mask term, the library and the oracle switched together (as in tests/test_gpu_geometry.py)."""
    from genpc_amd import _lib
    prev_l = _lib.lib.genpc_render_tune(request.param)
    prev_o = oracle.set_blend(request.param)
    yield request.param
    _lib.lib.genpc_render_tune(prev_l)
    oracle.set_blend(prev_o)


_INPUTS, _NEIGHBOURS, _REFS = {}, {}, {}


def _inputs(row):
    key = (row.seed, row.b, row.nc, row.np)          # (a Chamfer-only row shares its full row's clouds)
    if key not in _INPUTS:
        x = shapes.inputs(row)
        for a in x.values():
            a.setflags(write=False)
        _INPUTS[key] = x
    return _INPUTS[key]


def _neighbours(oracle, row):
    key = (row.seed, row.b, row.nc, row.np)
    if key not in _NEIGHBOURS:
        x = _inputs(row)
        out = []
        for e in range(row.b):
            opts = oracle.pose_transform(x["complete"][e], x["center"][e], x["params"][e])
            d1, d2, i1, i2 = oracle.chamfer_forward(opts[None], x["partial"][e][None], 1)
            out.append((d1[0], i1[0], d2[0], i2[0]))
        _NEIGHBOURS[key] = out
    return _NEIGHBOURS[key]


def _reference(oracle, row, blend, coloured):
    """-> (loss [b,4] (Chamfer only: [b,3]), grad [b,10], grad of the Chamfer half alone [b,10]), float64, from the composition
    the single-element tests use; the oracle's blend must be `blend` already (render_blend)."""
    key = (row.id, blend if row.mask else None, coloured)
    if key not in _REFS:
        x, nb = _inputs(row), _neighbours(oracle, row)
        lo_all, g_all, gcd_all = [], [], []
        for e in range(row.b):
            args = (x["complete"][e], x["center"][e], x["params"][e], x["partial"][e]) + nb[e]
            lo_cd, g_cd = oracle.pose_loss_grad(*args)
            if row.mask:
                ref = oracle.splat_image(x["partial"][e], row.radius, row.size, x["pcol"][e] if coloured else None)
                lo, g = oracle.pose_full_loss_grad(*args, row.radius, row.size, ref, vert_col=x["ccol"][e] if coloured else None)
            else:
                lo, g = lo_cd, g_cd
            lo_all.append(lo); g_all.append(g); gcd_all.append(g_cd)
        out = tuple(np.stack(a).astype(np.float64) for a in (lo_all, g_all, gcd_all))
        for a in out:
            a.setflags(write=False)
        _REFS[key] = out
    return _REFS[key]


def _assert_reference_speaks(row, lo, g, g_cd, tol):
    """What the comparison rests on, asserted on the reference alone: no two elements of the batch have the same total loss
    within the tolerance (an element mix-up shows), and the mask term carries weight in every element's gradient."""
    total = np.sort(lo[:, 0])
    gap = np.diff(total)
    assert (gap > tol["l_rtol"] * np.abs(total[1:]) + tol["l_atol"]).all(), (row.id, gap.min())
    if row.mask:
        for e in range(row.b):
            assert np.abs(g[e] - g_cd[e]).max() > 0.05 * np.abs(g[e]).max(), (row.id, e)


def _ratios(loss, grad, lo, g, tol):
    """Worst deviation / tolerance over the elements: of the loss vector, and of each gradient group."""
    loss, grad = np.asarray(loss, np.float64), np.asarray(grad, np.float64)
    out = [float((np.abs(loss - lo) / (tol["l_atol"] + tol["l_rtol"] * np.abs(lo))).max())]
    for sl in GROUPS:
        out.append(float((np.abs(grad[:, sl] - g[:, sl]).max(1) / (tol["g_rel"] * np.abs(g[:, sl]).max(1) + tol["g_abs"])).max()))
    return out


def _assert_close(what, loss, grad, lo, g, tol):
    assert np.isfinite(np.asarray(loss)).all() and np.isfinite(np.asarray(grad)).all(), what
    r = _ratios(loss, grad, lo, g, tol)
    print("deviation / tolerance  %-44s loss %.3f  grad[0:6] %.3f  grad[6:9] %.3f  grad[9] %.3f" % ((what,) + tuple(r)))
    np.testing.assert_allclose(loss, lo, rtol=tol["l_rtol"], atol=tol["l_atol"], err_msg=what)
    gg = np.asarray(grad, np.float64)
    for e in range(len(gg)):
        for sl in GROUPS:
            assert np.abs(gg[e, sl] - g[e, sl]).max() <= tol["g_rel"] * np.abs(g[e, sl]).max() + tol["g_abs"], (what, e, sl, gg[e, sl], g[e, sl])


def _run(gp, row, coloured, elements=None):
    torch, x = gp["torch"], _inputs(row)
    sel = slice(None) if elements is None else elements
    dev = {k: torch.from_numpy(np.ascontiguousarray(v[sel])).cuda() for k, v in x.items()}
    kw = dict(vert_col=dev["ccol"], partial_col=dev["pcol"]) if coloured and row.mask else {}
    if not row.mask:
        kw["mask_weight"] = 0.0
    loss, grad = gp["POSE"].pose_loss_grad_batch(dev["complete"], dev["center"], dev["params"], dev["partial"], row.radius, row.size, **kw)
    n = len(dev["params"])
    assert loss.shape == (n, 4) and grad.shape == (n, 10)
    return loss.cpu().numpy(), grad.cpu().numpy()


def _colourings(blend):
    # Pulsar's blend on white clouds: a hard rim, the mask term piecewise constant in the pose and its gradient exactly 0 -- the
    # comparison would say nothing; the coverage splat runs white and coloured
    return (True,) if blend == 1 else (False, True)


@pytest.mark.parametrize("row", shapes.FULL, ids=lambda r: r.id)
def test_full_objective_row_vs_oracle(gp, oracle, render_blend, row):
    for coloured in _colourings(render_blend):
        lo, g, g_cd = _reference(oracle, row, render_blend, coloured)
        _assert_reference_speaks(row, lo, g, g_cd, FULL_TOL)
        loss, grad = _run(gp, row, coloured)
        _assert_close("%s blend %d %s" % (row.id, render_blend, "coloured" if coloured else "white"), loss, grad, lo, g, FULL_TOL)


@pytest.mark.parametrize("row", shapes.CD_ONLY, ids=lambda r: r.id)
def test_chamfer_only_row_vs_oracle(gp, oracle, row):
    lo, g, g_cd = _reference(oracle, row, None, False)
    _assert_reference_speaks(row, lo, g, g_cd, CD_TOL)
    loss, grad = _run(gp, row, False)
    assert (loss[:, 3] == 0.0).all()          # no mask term
    _assert_close("%s Chamfer only" % row.id, loss[:, :3], grad, lo, g, CD_TOL)


def test_scratch_between_batch_sizes(gp, oracle, render_blend):
    """D, then B, then D again through the one workspace: 16 images of 128 x 128, 3 of 224 x 224, 16 again -- the tile counters
    and flags of a workspace last used with another batch size (MaskScratch::zero_bins).  The second D equals the first within
    the tolerances, and B still matches its oracle."""
    D, B = shapes.BY_ID["D"], shapes.BY_ID["B"]
    first = _run(gp, D, True)
    mid = _run(gp, B, True)
    second = _run(gp, D, True)
    lo, g, _ = _reference(oracle, D, render_blend, True)
    _assert_close("D first, blend %d" % render_blend, first[0], first[1], lo, g, FULL_TOL)
    lo_b, g_b, _ = _reference(oracle, B, render_blend, True)
    _assert_close("B between two D, blend %d" % render_blend, mid[0], mid[1], lo_b, g_b, FULL_TOL)
    _assert_close("D again vs D first, blend %d" % render_blend, second[0], second[1], first[0].astype(np.float64), first[1].astype(np.float64), FULL_TOL)
    _assert_close("D again, blend %d" % render_blend, second[0], second[1], lo, g, FULL_TOL)


def test_one_element_agrees_with_pose_loss_grad(gp, oracle, render_blend):
    """b = 1: the batched entry (projection in the transform's launch, the loop's own neighbour search) and pose_loss_grad
    (projection in the splat's launch pair, the caller's neighbours) on one element of G."""
    torch, G = gp["torch"], shapes.BY_ID["G"]
    x = _inputs(G)
    for coloured in _colourings(render_blend):
        for e in (0, G.b - 1):
            loss, grad = _run(gp, G, coloured, elements=slice(e, e + 1))
            kw = dict(vert_col=torch.from_numpy(x["ccol"][e]).cuda(), partial_col=torch.from_numpy(x["pcol"][e]).cuda()) if coloured else {}
            l1, g1 = gp["POSE"].pose_loss_grad(torch.from_numpy(x["complete"][e]).cuda(), torch.from_numpy(x["center"][e]).cuda(),
                                               torch.from_numpy(x["params"][e]).cuda(), torch.from_numpy(x["partial"][e]).cuda(), G.radius, G.size, **kw)
            l1, g1 = l1.cpu().numpy()[None], g1.cpu().numpy()[None]
            print("b = 1 vs pose_loss_grad, element %d, blend %d, %s: bit-equal loss %s, gradient %s"
                  % (e, render_blend, "coloured" if coloured else "white", np.array_equal(loss, l1), np.array_equal(grad, g1)))
            _assert_close("G[%d] alone vs pose_loss_grad, blend %d" % (e, render_blend), loss, grad, l1.astype(np.float64), g1.astype(np.float64), FULL_TOL)
            lo, g, _ = _reference(oracle, G, render_blend, coloured)
            _assert_close("G[%d] alone vs oracle, blend %d" % (e, render_blend), loss, grad, lo[e:e + 1], g[e:e + 1], FULL_TOL)


def test_wrapper_refuses_mismatched_shapes(gp):
    torch, POSE = gp["torch"], gp["POSE"]
    v, q = torch.rand(2, 300, 3).cuda(), torch.rand(2, 200, 3).cuda()
    c, p = v.mean(1), torch.from_numpy(np.stack([shapes.BASE_PARAMS] * 2)).cuda()
    with pytest.raises(ValueError):
        POSE.pose_loss_grad_batch(v, c, p, q, 0.02, 64, vert_col=torch.ones(2, 299, 3).cuda())
    with pytest.raises(ValueError):
        POSE.pose_loss_grad_batch(v, c, p, q, 0.02, 64, partial_col=torch.ones(1, 200, 3).cuda())
    with pytest.raises(ValueError):
        POSE.pose_loss_grad_batch(v, c, p[:1], q, 0.02, 64)
    with pytest.raises(ValueError):
        POSE.pose_loss_grad_batch(v, c[:1], p, q, 0.02, 64)
    with pytest.raises(ValueError):
        POSE.pose_loss_grad_batch(v, c, p, q[:1], 0.02, 64)
    with pytest.raises(ValueError):
        POSE.pose_loss_grad_batch(v[0], c, p, q, 0.02, 64)
    # what the library itself refuses (-1): an image of one pixel, a radius that is not positive -- with a mask term only
    with pytest.raises(RuntimeError, match="rc=-1"):
        POSE.pose_loss_grad_batch(v, c, p, q, 0.02, 1)
    with pytest.raises(RuntimeError, match="rc=-1"):
        POSE.pose_loss_grad_batch(v, c, p, q, 0.0, 64)
    loss, grad = POSE.pose_loss_grad_batch(v, c, p, q, 0.0, 0, mask_weight=0.0)
    assert torch.isfinite(loss).all() and torch.isfinite(grad).all() and float(loss[:, 3].abs().max()) == 0.0
