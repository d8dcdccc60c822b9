"""genpc_mask_loss -- mask_ref_kernel, mask_image_sums_kernel, mask_sums_kernel, mask_w_kernel on a caller's images -- against the
float64 oracle, per pixel and for the loss, on the cases of tests/mask_loss_cases.py: P from 4 to 513 x 513 (below and above a block
of either kind, not a multiple of the wave, through both grid-stride loops), constant, black, out-of-range and saturated content.
The bars are mask_loss_cases.image_bars: 8 x what the reference's own float32 formula shows against the same oracle."""
import numpy as np
import pytest

import mask_loss_cases as C

pytestmark = pytest.mark.gpu

CASES = C.image_cases()


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib
    from genpc_amd.optim_registration import diff_obj_pose as POSE
    return dict(torch=torch, POSE=POSE, lib=_lib)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_mask_loss_per_pixel(env, oracle, case):
    name, kind, S, img, ref = case
    torch, POSE = env["torch"], env["POSE"]
    a, r = torch.from_numpy(img).cuda(), torch.from_numpy(ref).cuda()
    loss, grad = POSE.mask_loss(a, r, with_grad=True)
    loss, grad = float(loss), grad.cpu().numpy()
    loss2, grad2 = POSE.mask_loss(a, r, with_grad=True)
    want_loss, want = oracle.mask_loss(img, ref, with_grad=True)
    t_abs, t_rel, t_loss = C.image_bars(kind)
    e_abs, e_rel = C.errors(grad, want)
    slack = C.shoulder_bound(img, ref) if kind == "shoulder" else 0.0
    print("%s: e_abs %.3g (bar %.3g)  e_rel %.3g (bar %.3g)  loss %.9g want %.9g: %.3g (bar %.3g + %.3g)"
          % (name, e_abs, t_abs, e_rel, t_rel, loss, want_loss, abs(loss - want_loss) / abs(want_loss), t_loss, slack / abs(want_loss)))
    assert np.isfinite(grad).all() and grad.shape == (S, S, 3)
    assert e_abs <= t_abs and e_rel <= t_rel, (name, e_abs, e_rel)
    assert abs(loss - want_loss) <= t_loss * abs(want_loss) + slack, (name, loss, want_loss)
    # the same call through the same workspace again: the same bits
    assert float(loss2) == loss and np.array_equal(grad2.cpu().numpy().view(np.uint32), grad.view(np.uint32)), name


def test_a_one_pixel_image_is_refused(env):
    torch, lib = env["torch"], env["lib"]
    a = torch.zeros(1, 1, 3, device="cuda")
    out = torch.full((4,), 7.0, device="cuda")
    rc = lib.on_device_of(a, lib.lib.genpc_mask_loss, 1, lib.ptr(a), lib.ptr(a), lib.ptr(out), lib.ptr(out[1:]))
    assert rc == -1 and (out == 7.0).all()
    with pytest.raises(RuntimeError, match="rc=-1"):
        env["POSE"].mask_loss(a, a)
