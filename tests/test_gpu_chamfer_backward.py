"""genpc_chamfer_backward on every path of its two kernels (csrc/chamfer.hip: chamfer_grad_kernel below 262144 points,
chamfer_grad_dir_kernel from there on) against tests/chamfer_grad_cases.py: `reference` is the plain statement of the
operation, `bound` the textbook rounding bound of an fp32 sum in any order, and tests/test_chamfer_grad_cases.py proves on
the CPU which paths every case reaches.  The gradients are pre-filled with `init`: the entry accumulates into what it is
handed, so what must come out is init + sums.  On the lattice flavour nothing rounds and the comparison has no tolerance: one
term lost, doubled or put on another row among 258048 fails it."""
import numpy as np
import pytest

import chamfer_grad_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gp():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib
    from genpc_amd.loss_functions import chamfer_3DDist
    return dict(torch=torch, lib=_lib, cd=chamfer_3DDist())


def backward(gp, c, gd1=None, gd2=None, calls=1, stream=None, split=False):
    """init1, init2 after `calls` calls of the entry on the case -> numpy.  split: one call per batch element."""
    torch, _lib = gp["torch"], gp["lib"]
    L, p = _lib.lib, _lib.ptr
    dev = lambda x: torch.from_numpy(np.array(x)).cuda()          # (a copy: the cases' arrays are read-only)
    A, B, I1, I2 = dev(c.xyz1), dev(c.xyz2), dev(c.idx1), dev(c.idx2)
    G1, G2 = dev(c.gd1 if gd1 is None else gd1), dev(c.gd2 if gd2 is None else gd2)
    ga, gb = dev(c.init1), dev(c.init2)

    def enqueue():
        for _ in range(calls):
            if split:
                for e in range(c.bsz):
                    s = slice(e, e + 1)
                    assert _lib.on_device_of(A, L.genpc_chamfer_backward, 1, c.n, p(A[s]), c.m, p(B[s]), p(G1[s]), p(I1[s]),
                                             p(G2[s]), p(I2[s]), p(ga[s]), p(gb[s])) == 1
            else:
                assert _lib.on_device_of(A, L.genpc_chamfer_backward, c.bsz, c.n, p(A), c.m, p(B), p(G1), p(I1), p(G2), p(I2),
                                         p(ga), p(gb)) == 1

    if stream is None:
        enqueue()
        torch.cuda.synchronize()
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            enqueue()
        stream.synchronize()
    return ga.cpu().numpy(), gb.cpu().numpy()


def assert_exact(got, exp, what):
    """As values (-0 equals +0), element by element; the message names the first rows that differ."""
    for g, e, cloud in zip(got, exp, ("gradxyz1", "gradxyz2")):
        bad = np.argwhere(g.astype(np.float64) != e)
        assert bad.size == 0, "%s %s: %d of %d elements differ, first at [batch, row, axis] %s: got %r, expected %r" % (
            what, cloud, len(bad), g.size, bad[0].tolist(), float(g[tuple(bad[0])]), float(e[tuple(bad[0])]))


def worst_ratio(got, exp, ks, Ss):
    """max |got - reference| / bound over both gradients (0 / 0 counts as 0: an element with nothing to round)."""
    worst = 0.0
    for g, e, k, S in zip(got, exp, ks, Ss):
        err, bnd = np.abs(g.astype(np.float64) - e), C.bound(k, S)
        assert np.isfinite(g).all()
        ratio = np.where(err == 0.0, 0.0, err / np.where(bnd > 0.0, bnd, 1.0))
        ratio = np.where((err > 0.0) & (bnd == 0.0), np.inf, ratio)
        worst = max(worst, float(ratio.max()))
    return worst


def assert_within_bound(got, name, what, exp=None):
    e, k, S = exp if exp is not None else C.expected(name, "float")
    w = worst_ratio(got, e, k, S)
    print("chamfer backward %s %s: worst |got - reference| / bound = %.4f" % (what, name, w))
    assert w <= 1.0, "%s %s: worst |got - reference| / bound = %.4f" % (what, name, w)
    return w


@pytest.mark.parametrize("name", C.CASES)
def test_lattice_every_case_is_exact(gp, name):
    assert_exact(backward(gp, C.case(name, "lattice")), C.expected(name, "lattice")[0], name)


@pytest.mark.parametrize("name", C.FLOAT_CASES)
def test_float_every_case_within_the_bound(gp, name):
    assert_within_bound(backward(gp, C.case(name, "float")), name, "float")


@pytest.mark.parametrize("name", C.OWN_ROW_CASES)
def test_float_own_rows_bit_for_bit(gp, name):
    """With the other direction's weights zero a gradient is fl(init + v), v = fl(fl(2 gd) fl(q - t)): one multiply, a
    separate subtract and one rounded add, nothing contracted -- on both kernels."""
    c = C.case(name, "float")
    ga, _ = backward(gp, c, gd2=np.zeros_like(c.gd2))
    exp = (c.init1 + C.terms(c.xyz1, c.xyz2, c.gd1, c.idx1)).astype(np.float32)
    assert np.array_equal(ga, exp), "%s gradxyz1: %d elements differ" % (name, int((ga != exp).sum()))
    _, gb = backward(gp, c, gd1=np.zeros_like(c.gd1))
    exp = (c.init2 + C.terms(c.xyz2, c.xyz1, c.gd2, c.idx2)).astype(np.float32)
    assert np.array_equal(gb, exp), "%s gradxyz2: %d elements differ" % (name, int((gb != exp).sum()))


def test_both_kernels_on_one_problem(gp):
    """batch8 as one call takes the tile kernel, as eight one-element calls the atomic kernel."""
    c = C.case("batch8", "lattice")
    assert c.bsz * (c.n + c.m) >= C.THRESHOLD > c.n + c.m
    one, eight = backward(gp, c), backward(gp, c, split=True)
    assert_exact(one, C.expected("batch8", "lattice")[0], "batch8 in one call")
    assert_exact(eight, C.expected("batch8", "lattice")[0], "batch8 in eight calls")
    assert np.array_equal(one[0], eight[0]) and np.array_equal(one[1], eight[1])
    c = C.case("batch8", "float")
    assert_within_bound(backward(gp, c), "batch8", "one call")
    assert_within_bound(backward(gp, c, split=True), "batch8", "eight calls")


def test_side_stream_and_second_accumulation(gp):
    torch = gp["torch"]
    c = C.case("batch16", "lattice")
    (e1, e2), _, _ = C.expected("batch16", "lattice")
    assert_exact(backward(gp, c, stream=torch.cuda.Stream()), (e1, e2), "batch16 on a side stream")
    # twice into the same buffers: init + 2 sums (exact: the lattice leaves a factor 2 of headroom, asserted here)
    twice = tuple(2.0 * e - i.astype(np.float64) for e, i in ((e1, c.init1), (e2, c.init2)))
    S = C.expected("batch16", "lattice")[2]
    assert 2.0 * max(S[0].max(), S[1].max()) / C.QUANTUM < 2 ** 24
    assert_exact(backward(gp, c, calls=2), twice, "batch16 called twice")
    assert_exact(backward(gp, c, calls=2, stream=torch.cuda.Stream()), twice, "batch16 called twice on a side stream")


def test_through_autograd_at_the_threshold(gp):
    """chamfer_3DDist on 2 x 65536 x 65536 (262144 points: the tile kernel), the indices the forward's own."""
    torch = gp["torch"]
    from conftest import gen_pair
    bsz, n = 2, 65536
    assert bsz * 2 * n == C.THRESHOLD
    a, b = gen_pair(41, (bsz, n, 3), (bsz, n, 3))
    rng = np.random.default_rng(42)
    w1, w2 = rng.random((bsz, n), dtype=np.float32), rng.random((bsz, n), dtype=np.float32)
    A, B = torch.from_numpy(a).cuda().requires_grad_(True), torch.from_numpy(b).cuda().requires_grad_(True)
    d1, d2, i1, i2 = gp["cd"](A, B)
    ((d1 * torch.from_numpy(w1).cuda()).sum() + (d2 * torch.from_numpy(w2).cuda()).sum()).backward()
    i1, i2 = i1.cpu().numpy(), i2.cpu().numpy()
    assert i1.min() >= 0 and i1.max() < n and i2.min() >= 0 and i2.max() < n
    zero = np.zeros_like(a)
    assert_within_bound((A.grad.cpu().numpy(), B.grad.cpu().numpy()), "2x65536x65536", "autograd",
                        exp=C.reference(a, b, w1, w2, i1, i2, zero, zero))
    # a loss on d1 alone, xyz1 alone requiring grad: its gradient is the term itself
    A2 = torch.from_numpy(a).cuda().requires_grad_(True)
    e1, _, j1, _ = gp["cd"](A2, torch.from_numpy(b).cuda())
    (e1 * torch.from_numpy(w1).cuda()).sum().backward()
    assert np.array_equal(j1.cpu().numpy(), i1)
    exp = C.terms(a, b, w1, i1)
    got = A2.grad.cpu().numpy()
    assert np.array_equal(got, exp), "%d elements differ" % int((got != exp).sum())
