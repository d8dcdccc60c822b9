"""chamfer_raggedDist / chamfer_raggedFunction (loss_functions/Chamfer3D/dist_chamfer_ragged.py) and chamfer_ragged_loss
(utils/loss_util.py) on the GPU: the gradients that reach the caller's tensors are the library's, bit for bit; against the
rectangular chamfer_3DDist they agree at that kernel's own bar (its atomics fix no order)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES1 = [300, 1, 1025, 64, 777]
SIZES2 = [513, 3000, 2, 65, 777]


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib, chamfer_3D
    from genpc_amd.loss_functions.Chamfer3D import dist_chamfer_ragged as ragged
    return dict(torch=torch, L=_lib, ch=chamfer_3D, ragged=ragged)


def uniform(rng, n):
    return rng.random((n, 3), dtype=np.float32) - np.float32(0.5)


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def test_list_and_packed_gradients_are_the_library_s_bits(env):
    torch, ragged = env["torch"], env["ragged"]
    rng = np.random.default_rng(31)
    c1 = [torch.from_numpy(uniform(rng, n)).cuda().requires_grad_(True) for n in SIZES1]
    c2 = [torch.from_numpy(uniform(rng, m)).cuda().requires_grad_(True) for m in SIZES2]
    w1 = torch.from_numpy(rng.normal(size=sum(SIZES1)).astype(np.float32)).cuda()
    w2 = torch.from_numpy(rng.normal(size=sum(SIZES2)).astype(np.float32)).cuda()
    d1, d2, i1, i2, o1, o2 = ragged.chamfer_raggedDist()(c1, c2)
    assert d1.requires_grad and d2.requires_grad and not i1.requires_grad and not i2.requires_grad
    assert o1.tolist() == [0] + list(np.cumsum(SIZES1)) and o2.tolist() == [0] + list(np.cumsum(SIZES2))
    f1, f2, j1, j2, _, _ = ragged.chamfer_ragged([t.detach() for t in c1], [t.detach() for t in c2])
    assert np.array_equal(bits(d1), bits(f1)) and np.array_equal(bits(d2), bits(f2))
    assert torch.equal(i1, j1) and torch.equal(i2, j2)
    ((w1 * d1).sum() + (w2 * d2).sum()).backward()

    # the direct call: the weights ARE the gradients of the distances
    P1, P2 = torch.cat([t.detach() for t in c1]).contiguous(), torch.cat([t.detach() for t in c2]).contiguous()
    g1 = torch.full_like(P1, float("nan"))
    g2 = torch.full_like(P2, float("nan"))
    assert env["ch"].backward_ragged(P1, o1, P2, o2, g1, g2, w1, w2, i1, i2) == 1, env["L"].last_error()
    for cs, g, off in ((c1, g1, o1.tolist()), (c2, g2, o2.tolist())):
        for j, t in enumerate(cs):
            assert t.grad is not None and np.array_equal(bits(t.grad), bits(g[off[j]:off[j + 1]])), "list element %d" % j

    # the packed form
    Q1, Q2 = P1.clone().requires_grad_(True), P2.clone().requires_grad_(True)
    e1, e2, _, _, _, _ = ragged.chamfer_raggedDist()((Q1, o1), (Q2, o2.tolist()))
    ((w1 * e1).sum() + (w2 * e2).sum()).backward()
    assert np.array_equal(bits(Q1.grad), bits(g1)) and np.array_equal(bits(Q2.grad), bits(g2))


def test_rectangular_input_agrees_with_chamfer_3DDist(env):
    torch, ragged = env["torch"], env["ragged"]
    from genpc_amd.loss_functions import chamfer_3DDist
    rng = np.random.default_rng(32)
    a, b = rng.random((3, 1000, 3), dtype=np.float32) - np.float32(0.5), rng.random((3, 777, 3), dtype=np.float32) - np.float32(0.5)
    w1 = torch.from_numpy(rng.normal(size=(3, 1000)).astype(np.float32)).cuda()
    w2 = torch.from_numpy(rng.normal(size=(3, 777)).astype(np.float32)).cuda()
    A, B = torch.from_numpy(a).cuda().requires_grad_(True), torch.from_numpy(b).cuda().requires_grad_(True)
    d1, d2, _, _ = chamfer_3DDist()(A, B)
    ((w1 * d1).sum() + (w2 * d2).sum()).backward()
    RA = [torch.from_numpy(a[j]).cuda().requires_grad_(True) for j in range(3)]
    RB = [torch.from_numpy(b[j]).cuda().requires_grad_(True) for j in range(3)]
    e1, e2, _, _, _, _ = ragged.chamfer_raggedDist()(RA, RB)
    assert np.array_equal(bits(e1).reshape(3, 1000), bits(d1)) and np.array_equal(bits(e2).reshape(3, 777), bits(d2))
    ((w1.reshape(-1) * e1).sum() + (w2.reshape(-1) * e2).sum()).backward()
    for j in range(3):
        np.testing.assert_allclose(RA[j].grad.cpu().numpy(), A.grad[j].cpu().numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(RB[j].grad.cpu().numpy(), B.grad[j].cpu().numpy(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("kind", ["l1", "l2"])
def test_chamfer_ragged_loss_against_completionloss_per_pair(env, kind):
    """fp32 means of Completionloss against float64 segment means cast to fp32: (log2 N + a few) 2^-24 at these sizes is about
    1e-6 (tests/test_gpu_nn_ragged.py); the bar, with its tenfold margin, is 1e-5.  The gradients inherit the factor 1 / N of
    the means and, for l1, 1 / (2 sqrt d) in fp32 on both sides; the per-pair loop accumulates with chamfer_3DDist's atomics,
    held to 1e-5 relative itself."""
    torch = env["torch"]
    from genpc_amd.utils.loss_util import Completionloss, chamfer_ragged_loss
    rng = np.random.default_rng(33)
    a = [uniform(rng, n) for n in SIZES1]
    b = [uniform(rng, m) for m in SIZES2]
    c1 = [torch.from_numpy(x).cuda().requires_grad_(True) for x in a]
    c2 = [torch.from_numpy(x).cuda().requires_grad_(True) for x in b]
    w = torch.from_numpy(rng.random(len(a)).astype(np.float32) + np.float32(0.5)).cuda()
    loss = chamfer_ragged_loss(c1, c2, kind)
    assert loss.dtype == torch.float32 and tuple(loss.shape) == (len(a),)
    (w * loss).sum().backward()
    ref = Completionloss("cd_" + kind)
    for j in range(len(a)):
        x = torch.from_numpy(a[j]).cuda()[None].requires_grad_(True)
        y = torch.from_numpy(b[j]).cuda()[None].requires_grad_(True)
        one = ref.get_loss(x, y)
        (w[j] * one).backward()
        print("pair %d %s: loss %.8g against %.8g, relative difference %.3g" % (j, kind, loss[j].item(), one.item(), abs(loss[j].item() / one.item() - 1)))
        np.testing.assert_allclose(loss[j].item(), one.item(), rtol=1e-5, atol=0)
        for got, want, name in ((c1[j].grad, x.grad[0], "clouds1"), (c2[j].grad, y.grad[0], "clouds2")):
            got, want = got.cpu().numpy(), want.cpu().numpy()
            print("   grad %s: max abs difference %.3g of max %.3g" % (name, np.abs(got - want).max(), np.abs(want).max()))
            np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())
