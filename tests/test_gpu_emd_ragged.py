"""The ragged auction EMD (csrc/emd_ragged.hip: genpc_emd_forward_ragged / genpc_emd_backward_ragged, emd_raggedDist,
emd_ragged_loss, metric.evaluate_scans_ragged) on the GPU.  Per pair, dist, assignment, assignment_inv, bid and
bid_increments are compared BIT FOR BIT with the CPU oracle on that pair alone and with the dense library call on that pair
alone, in both arithmetic modes; price at the bar tests/test_gpu_emd.py uses (exact except after a forced last round with
several bidders on one object).  The outputs of a ragged call are allocated UNINITIALISED (filled with garbage here): the
call's first launch owns the initial state.

Launch count: a call enqueues 2 * iters + 2 launches (include/genpc_hip.h); there is no cheap way to count
launches without a profiler, so no test asserts it."""
import numpy as np
import pytest

from conftest import gen_pair

pytestmark = pytest.mark.gpu

FIVE = ("assignment", "dist", "assignment_inv", "bid", "bid_increments")
SIZES = [256, 1024, 0, 768, 2304, 512, 1280]          # both sides of the 1024- and of the 2048-object tile, an empty pair


@pytest.fixture(scope="module")
def gp():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib, emd, metric
    from genpc_amd.loss_functions import emdModule, emd_raggedDist
    from genpc_amd.loss_functions.emd.emd_module import alloc_state
    from genpc_amd.utils.loss_util import Completionloss, emd_ragged_loss
    return dict(torch=torch, lib=_lib, emd=emd, metric=metric, mod=emdModule(), rag=emd_raggedDist(), alloc=alloc_state,
                CL=Completionloss, loss=emd_ragged_loss)


def make_pairs(sizes, seed):
    """One (points, objects) pair of [n,3] float32 arrays per size, from conftest.gen_pair."""
    return [gen_pair(seed + 31 * j, (n, 3), (n, 3), 0.0) for j, n in enumerate(sizes)]


def offsets(pairs):
    off = [0]
    for a, _ in pairs:
        off.append(off[-1] + a.shape[0])
    return off


class Arith:
    def __init__(self, gp, mode):
        self.lib, self.mode = gp["lib"].lib, mode

    def __enter__(self):
        self.prev = self.lib.genpc_set_arith(self.mode)

    def __exit__(self, *exc):
        self.lib.genpc_set_arith(self.prev)


def garbage_state(gp, total):
    """The eight state arrays of a ragged call, filled with values no initial state has."""
    torch = gp["torch"]
    f = lambda: torch.full((total,), 123.25, dtype=torch.float32, device="cuda")
    i = lambda: torch.full((total,), 77, dtype=torch.int32, device="cuda")
    return dict(dist=f(), price=f(), bid_increments=f(), max_increments=f(), assignment=i(), assignment_inv=i(), bid=i(), max_idx=i())


def run_ragged(gp, pairs, eps, iters, mode, state=None, expect_rc=1):
    """One ragged call; returns the state arrays as numpy, packed, and the offsets."""
    torch = gp["torch"]
    off = offsets(pairs)
    A = torch.from_numpy(np.concatenate([a for a, _ in pairs] + [np.zeros((0, 3), np.float32)])).cuda()
    B = torch.from_numpy(np.concatenate([b for _, b in pairs] + [np.zeros((0, 3), np.float32)])).cuda()
    s = state if state is not None else garbage_state(gp, off[-1])
    with Arith(gp, mode):
        rc = gp["emd"].forward_ragged(A, B, off, s["dist"], s["assignment"], s["price"], s["assignment_inv"], s["bid"],
                                      s["bid_increments"], s["max_increments"], s["max_idx"], eps, iters)
        torch.cuda.synchronize()
    assert rc == expect_rc, gp["lib"].last_error()
    return {k: v.cpu().numpy() for k, v in s.items()}, off


def run_dense(gp, a, b, eps, iters, mode, tune):
    """genpc_emd_forward on one pair alone, from alloc_state's initial values, with the given bid implementation."""
    torch = gp["torch"]
    prev = gp["lib"].lib.genpc_emd_tune(tune, -1)
    try:
        with Arith(gp, mode):
            A, B = torch.from_numpy(a[None]).cuda(), torch.from_numpy(b[None]).cuda()
            s = gp["alloc"](1, a.shape[0], b.shape[0], A.device)
            rc = gp["emd"].forward(A, B, s["dist"], s["assignment"], s["price"], s["assignment_inv"], s["bid"], s["bid_increments"],
                                   s["max_increments"], s["unass_idx"], s["unass_cnt"], s["unass_cnt_sum"], s["cnt_tmp"], s["max_idx"],
                                   eps, iters)
            torch.cuda.synchronize()
        assert rc == 1
    finally:
        gp["lib"].lib.genpc_emd_tune(prev, -1)
    return {k: v.cpu().numpy().reshape(-1) for k, v in s.items()}


_ORACLE = {}


def oracle_pair(oracle, key, a, b, eps, iters, mode):
    """The oracle's state on one pair alone; computed once per (key, eps, iters, mode) and shared, never modified."""
    k = (key, float(eps), int(iters), int(mode))
    if k not in _ORACLE:
        d, ass, st = oracle.emd_forward(a[None], b[None], eps, iters, mode, return_state=True)
        st = {n: np.ascontiguousarray(v).reshape(-1) for n, v in st.items()}
        for v in st.values():
            v.setflags(write=False)
        _ORACLE[k] = st
    return _ORACLE[k]


def check_against_oracle(oracle, got, off, pairs, key, eps, iters, mode, skip=()):
    for j, (a, b) in enumerate(pairs):
        if a.shape[0] == 0 or j in skip:
            continue
        st = oracle_pair(oracle, (key, j, a.shape[0]), a, b, eps, iters, mode)
        lo, hi = off[j], off[j + 1]
        for name in FIVE:
            np.testing.assert_array_equal(got[name][lo:hi], st[name], err_msg="pair %d (%d points) %s" % (j, hi - lo, name))
        np.testing.assert_allclose(got["price"][lo:hi], st["price"], rtol=1e-5, atol=2e-6, err_msg="pair %d price" % j)


@pytest.mark.parametrize("iters", [1, 2, 17, 50])
@pytest.mark.parametrize("mode", [0, 1])
def test_1_against_the_oracle(gp, oracle, iters, mode):
    pairs = make_pairs(SIZES, 100)
    got, off = run_ragged(gp, pairs, 0.005, iters, mode)
    check_against_oracle(oracle, got, off, pairs, "t1", 0.005, iters, mode)


@pytest.mark.parametrize("tune", [0, 1], ids=["tiled_bid", "culled_bid"])
@pytest.mark.parametrize("mode", [0, 1])
def test_2_against_the_dense_library(gp, mode, tune):
    pairs = make_pairs(SIZES, 100)
    got, off = run_ragged(gp, pairs, 0.005, 50, mode)
    for j, (a, b) in enumerate(pairs):
        if a.shape[0] == 0:
            continue
        d = run_dense(gp, a, b, 0.005, 50, mode, tune)
        for name in FIVE:
            np.testing.assert_array_equal(got[name][off[j]:off[j + 1]], d[name], err_msg="pair %d %s" % (j, name))


@pytest.mark.parametrize("mode", [0, 1])
def test_3_position_independence(gp, mode):
    """A pair's bits do not depend on where it stands in the call, nor on what stands beside it (its run of workgroups, its
    lanes per bidder and the tile length all change with the company)."""
    probe = gen_pair(7, (768, 3), (768, 3), 0.0)
    others = make_pairs([256, 1024, 2304], 300)
    seen = []
    for pos in (0, 1, 3):
        pairs = others[:pos] + [probe] + others[pos:]
        if pos == 1:
            pairs = pairs + make_pairs([4352], 400)        # more than 8192 points in the call: the 1024-object tile
        got, off = run_ragged(gp, pairs, 0.005, 30, mode)
        seen.append({name: got[name][off[pos]:off[pos + 1]].copy() for name in FIVE})
    for other in seen[1:]:
        for name in FIVE:
            np.testing.assert_array_equal(seen[0][name].view(np.uint32), other[name].view(np.uint32), err_msg=name)


@pytest.mark.parametrize("mode", [0, 1])
def test_4_ties(gp, oracle, golden, mode):
    """Duplicated points (exact first-place ties: the reference's thread-major order, from the pair's OWN N_j and bidder
    count, decides every index) and a pair whose two clouds are the same array."""
    g = golden("emd_seed5_dups.npz")
    same = gen_pair(11, (768, 3), (768, 3), 0.0)[0]
    pairs = [(g["xyz1"][0].copy(), g["xyz2"][0].copy()), (same, same.copy()), (g["xyz1"][1].copy(), g["xyz2"][1].copy())]
    for iters in (3, 50):
        got, off = run_ragged(gp, pairs, 0.005, iters, mode)
        check_against_oracle(oracle, got, off, pairs, "t4", 0.005, iters, mode)
    # the fixture's own recorded results for its 50 rounds
    np.testing.assert_array_equal(got["assignment"][off[0]:off[1]], g["assignment_m%d" % mode][0])
    np.testing.assert_array_equal(got["dist"][off[2]:off[3]], g["dist_m%d" % mode][1])


@pytest.mark.parametrize("mode", [0, 1])
def test_5_negative_eps_and_zero_rounds(gp, oracle, mode):
    pairs = make_pairs([512, 0, 1280, 256], 500)
    got, off = run_ragged(gp, pairs, -0.0005, 6, mode)
    check_against_oracle(oracle, got, off, pairs, "t5", -0.0005, 6, mode)
    got, off = run_ragged(gp, pairs, 0.005, 0, mode)            # rc == 1 is asserted inside
    assert (got["dist"] == 0).all() and (got["assignment"] == -1).all()
    assert (got["assignment_inv"] == -1).all() and (got["price"] == 0).all() and (got["bid"] == 0).all()


def test_6_the_pair_count_limit(gp, oracle):
    a, b = gen_pair(600, (384, 256, 3), (384, 256, 3), 0.0)
    pairs = [(a[j], b[j]) for j in range(384)]
    got, off = run_ragged(gp, pairs, 0.005, 5, 1)
    d, ass, st = oracle.emd_forward(a, b, 0.005, 5, 1, return_state=True)      # the oracle treats batch elements one by one
    for name in FIVE:
        np.testing.assert_array_equal(got[name].reshape(384, 256), np.asarray(st[name]).reshape(384, 256), err_msg=name)
    np.testing.assert_allclose(got["price"].reshape(384, 256), st["price"], rtol=1e-5, atol=2e-6)
    # one pair more is refused, nothing is written
    s = garbage_state(gp, 385 * 256)
    torch = gp["torch"]
    z = torch.zeros(385 * 256, 3, device="cuda")
    rc = gp["emd"].forward_ragged(z, z, list(range(0, 386 * 256, 256)), s["dist"], s["assignment"], s["price"], s["assignment_inv"],
                                  s["bid"], s["bid_increments"], s["max_increments"], s["max_idx"], 0.005, 5)
    torch.cuda.synchronize()
    assert rc == -1 and "more than 384 pairs" in gp["lib"].last_error()
    assert bool((s["assignment"] == 77).all()) and bool((s["dist"] == 123.25).all())


def test_6a_more_pairs_than_one_call_takes(gp, oracle):
    """emd_raggedDist splits a list of more than 384 pairs into several library calls, forward and backward: 386 pairs, the
    last two in a call of their own; results and gradients as the oracle has them for every pair."""
    torch = gp["torch"]
    c = 386
    a, b = gen_pair(650, (c, 256, 3), (c, 256, 3), 0.0)
    off = list(range(0, (c + 1) * 256, 256))
    P1 = torch.from_numpy(a.reshape(-1, 3)).cuda().requires_grad_(True)
    P2 = torch.from_numpy(b.reshape(-1, 3)).cuda()
    with Arith(gp, 1):
        dist, ass = gp["rag"]((P1, off), (P2, off), 0.005, 4)
        g = np.random.default_rng(4).random(c * 256, dtype=np.float32)
        (dist * torch.from_numpy(g).cuda()).sum().backward()
    d, oass = oracle.emd_forward(a, b, 0.005, 4, 1)
    np.testing.assert_array_equal(ass.cpu().numpy().reshape(c, 256), oass)
    np.testing.assert_array_equal(dist.detach().cpu().numpy().reshape(c, 256), d)
    np.testing.assert_array_equal(P1.grad.cpu().numpy().reshape(c, 256, 3), oracle.emd_backward(a, b, g.reshape(c, 256), oass))


def test_7_one_larger_pair_among_small_ones(gp, oracle):
    pairs = make_pairs([4352, 256, 256], 700)
    got, off = run_ragged(gp, pairs, 0.005, 50, 1)
    check_against_oracle(oracle, got, off, pairs, "t7", 0.005, 50, 1)


@pytest.mark.parametrize("mode", [0, 1])
def test_8_non_finite_coordinates(gp, oracle, mode):
    """A pair with an infinite and a NaN OBJECT equals the dense call on it alone (a non-finite BIDDER bids on object -1 in
    the reference -- an out-of-bounds write there and in the dense call: not run); its neighbours keep the oracle's results."""
    pairs = make_pairs([512, 1024, 768], 800)
    bad = pairs[1][1].copy()
    bad[5, 1] = np.inf
    bad[100, 0] = np.nan
    pairs[1] = (pairs[1][0], bad)
    got, off = run_ragged(gp, pairs, 0.005, 12, mode)
    check_against_oracle(oracle, got, off, pairs, "t8", 0.005, 12, mode, skip=(1,))
    d = run_dense(gp, pairs[1][0], bad, 0.005, 12, mode, 0)
    for name in FIVE:
        np.testing.assert_array_equal(got[name][off[1]:off[2]].view(np.uint32), d[name].view(np.uint32), err_msg=name)


@pytest.mark.parametrize("mode", [0, 1])
def test_8a_non_finite_bidder(gp, oracle, mode):
    """A BIDDER with a NaN coordinate, in the middle pair: none of its candidates compares above -1e9, and it bids on object 0
    of its own pair (csrc/emd_ragged.hip; the reference's object -1 would be a slot of the pair in front).  Its neighbours keep
    the oracle's bits, and every index the pair holds stays inside the pair."""
    pairs = make_pairs([256, 256, 256], 850)
    bad = pairs[1][0].copy()
    bad[97, 2] = np.nan
    pairs[1] = (bad, pairs[1][1])
    got, off = run_ragged(gp, pairs, 0.005, 3, mode)
    check_against_oracle(oracle, got, off, pairs, "t8a", 0.005, 3, mode, skip=(1,))
    assert got["bid"][off[1] + 97] == 0
    for name in ("bid", "assignment", "assignment_inv"):
        v = got[name][off[1]:off[2]]
        assert ((v >= -1) & (v < 256)).all(), name


def test_9_repeat_on_the_same_output_buffers(gp):
    pairs = make_pairs([768, 0, 2304, 256], 900)
    s = garbage_state(gp, offsets(pairs)[-1])
    first, off = run_ragged(gp, pairs, 0.005, 20, 1, state=s)
    first = {k: v.copy() for k, v in first.items()}
    second, _ = run_ragged(gp, pairs, 0.005, 20, 1, state=s)       # the state is what the first call left: nothing refilled
    for name in FIVE:
        np.testing.assert_array_equal(first[name].view(np.uint32), second[name].view(np.uint32), err_msg=name)


def test_10_backward(gp, oracle):
    torch = gp["torch"]
    sizes = [512, 0, 1280, 256]
    pairs = make_pairs(sizes, 1000)
    off = offsets(pairs)
    rng = np.random.default_rng(3)
    # the C entry point against the oracle, pair by pair, with assignments of its own forward
    got, _ = run_ragged(gp, pairs, 0.005, 30, 1)
    gd = rng.random(off[-1], dtype=np.float32)
    A = torch.from_numpy(np.concatenate([a for a, _ in pairs])).cuda()
    B = torch.from_numpy(np.concatenate([b for _, b in pairs])).cuda()
    gx = torch.zeros_like(A)
    rc = gp["emd"].backward_ragged(A, B, off, gx, torch.from_numpy(gd).cuda(), torch.from_numpy(got["assignment"]).cuda())
    torch.cuda.synchronize()
    assert rc == 1
    gx = gx.cpu().numpy()
    for j, (a, b) in enumerate(pairs):
        if a.shape[0] == 0:
            continue
        lo, hi = off[j], off[j + 1]
        e = oracle.emd_backward(a[None], b[None], gd[None, lo:hi], got["assignment"][None, lo:hi])
        np.testing.assert_array_equal(gx[lo:hi], e[0], err_msg="pair %d" % j)
    # through autograd: every element of the first list gets emdModule's gradient on that pair alone, the second list zeros
    c1 = [torch.from_numpy(a).cuda().requires_grad_(True) for a, _ in pairs]
    c2 = [torch.from_numpy(b).cuda().requires_grad_(True) for _, b in pairs]
    dist, ass = gp["rag"](c1, c2, 0.005, 30)
    assert isinstance(dist, list) and len(dist) == len(sizes) and [d.shape[0] for d in dist] == sizes
    assert all(not t.requires_grad and t.dtype == torch.int32 for t in ass)
    sum(torch.sqrt(d).sum() for d in dist).backward()
    for j, (a, b) in enumerate(pairs):
        if a.shape[0] == 0:
            assert c1[j].grad is None or c1[j].grad.numel() == 0
            continue
        x = torch.from_numpy(a[None]).cuda().requires_grad_(True)
        d, asg = gp["mod"](x, torch.from_numpy(b[None]).cuda(), 0.005, 30)
        torch.sqrt(d).sum().backward()
        assert torch.equal(asg[0], ass[j]) and torch.equal(d[0].detach(), dist[j].detach())
        assert torch.equal(c1[j].grad, x.grad[0]), "pair %d" % j
        assert c2[j].grad is not None and not bool(c2[j].grad.any())
    # packed in, packed out, the gradient on the packed points
    P1 = torch.from_numpy(np.concatenate([a for a, _ in pairs])).cuda().requires_grad_(True)
    dist_p, ass_p = gp["rag"]((P1, off), (B, off), 0.005, 30)
    assert torch.is_tensor(dist_p) and dist_p.shape == (off[-1],) and torch.equal(ass_p, torch.cat(ass))
    torch.sqrt(dist_p).sum().backward()
    assert torch.equal(P1.grad, torch.cat([t.grad for t in c1]))


def test_11_loss_and_metric(gp, oracle):
    torch = gp["torch"]
    sizes = [512, 1280, 256, 2304]
    pairs = make_pairs(sizes, 1100)
    c1 = [torch.from_numpy(a).cuda() for a, _ in pairs]
    c2 = [torch.from_numpy(b).cuda() for _, b in pairs]
    with Arith(gp, 1):
        loss = gp["loss"](c1, c2)
        assert loss.shape == (len(sizes),) and loss.dtype == torch.float32
        for j in range(len(sizes)):
            alone = gp["CL"]("emd").emd_loss(c1[j][None], c2[j][None])
            assert loss[j].item() == alone.item(), (j, loss[j].item(), alone.item())
        # evaluate_clouds accumulates its float64 means with atomic additions, whose order is free: under torch's
        # deterministic algorithms both evaluations add in one fixed order, and columns 0-1 can be compared exactly
        det = torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(True)
        try:
            m = gp["metric"].evaluate_scans_ragged(c1, c2)
            cd = gp["metric"].evaluate_clouds(c1, c2)
        finally:
            torch.use_deterministic_algorithms(det)
    assert m.shape == (len(sizes), 3) and m.dtype == torch.float64 and m.is_cuda
    assert torch.equal(m[:, :2], cd)
    want = [np.sqrt(oracle_pair(oracle, ("t11", j, a.shape[0]), a, b, 0.005, 50, 1)["dist"].astype(np.float64)).mean()
            for j, (a, b) in enumerate(pairs)]
    np.testing.assert_allclose(m[:, 2].cpu().numpy(), np.array(want), rtol=1e-9, atol=0)
