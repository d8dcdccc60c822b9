"""genpc_icp_batch_ragged / reg_xyz.registration_icp_ragged on the GPU.

A candidate of a pair whose target gets the one-workgroup plan must come out as the BITS of registration_icp on that pair alone
(np.array_equal on T, fitness, rmse and iterations), in both arithmetic modes: the kernel is the same device function, its
reductions are in fixed order, and its grid depends on the target, max_dist and the pair's own cell budget only.  A pair beyond
the one-workgroup limit runs through genpc_icp_batch's loop inside the same call and is held to that path's bars against
oracle.icp (tests/test_gpu_icp_paths.py): fitness and iterations equal, T within 1e-6 max(1, |tgt|max), rmse within 1e-7.
The target counts come from genpc_icp_plan (icp_pass_ref.path_sizes), so a change of a constant moves the tests with it; the
clouds are synthetic: two samplings of a box's surface, the source turned by a few degrees, moved, and 1.1 times smaller."""
import ctypes

import numpy as np
import pytest

import icp_pass_ref as R
from test_gpu_icp import rot
from test_gpu_icp_paths import library_modes

pytestmark = pytest.mark.gpu

MD = 0.075
HALF = np.array([0.5, 0.3, 0.2])


@pytest.fixture(scope="module")
def rg():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib, reg_xyz
    return dict(torch=torch, R=reg_xyz, lib=_lib.lib, L=_lib)


def box_surface(seed, n):
    """n points on the surface of the box [-0.5, 0.5] x [-0.3, 0.3] x [-0.2, 0.2]."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1.0, 1.0, (n, 3))
    axis = rng.integers(0, 3, n)
    p[np.arange(n), axis] = rng.choice([-1.0, 1.0], n)
    return (p * HALF).astype(np.float32)


def pair(seed, ns, nt):
    """(source, target): another sampling of the target's surface, turned by 4 degrees, moved and scaled by 1 / 1.1."""
    tgt = box_surface(seed, nt)
    Rm, t = rot([0.3, 1.0, -0.2], 4.0), np.array([0.015, -0.01, 0.02])
    src = ((box_surface(seed + 500, ns).astype(np.float64) / 1.1 - t) @ Rm).astype(np.float32)
    return src, tgt


def ragged_plan(rg, nts):
    toff = (ctypes.c_int * (len(nts) + 1))(*([0] + [int(v) for v in np.cumsum(nts)]))
    out = (ctypes.c_int * 3)(-1, -1, -1)
    assert rg["lib"].genpc_icp_ragged_plan(len(nts), ctypes.cast(toff, ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p)) == 1
    return tuple(out)


def fused_pairs():
    """(ns, nt, K) of one call whose pairs all get the one-workgroup plan, from different cell budgets: nt = 1, a 4k + 1 (the
    cloud's padding to a multiple of four), a mid-size one, the largest of the 4096-cell and of the 1024-cell budget; one pair
    without candidates."""
    budgets, first_loop = R.path_sizes()
    assert len(budgets) == 4 and budgets[-1][0] == 1024 and budgets[-1][1] + 1 == first_loop
    return [(63, 1, 3), (1, 1001, 1), (100, 500, 0), (1999, 3001, 11), (257, budgets[1][1], 1), (1025, budgets[-1][1], 3)]


def make(pairs, seed=0):
    clouds = [pair(seed + 10 * j, ns, nt) for j, (ns, nt, _) in enumerate(pairs)]
    inits = [np.array(R.inits(seed + j, max(k, 1))[:k]).reshape(k, 4, 4) for j, (_, _, k) in enumerate(pairs)]
    return clouds, inits


def to_dev(rg, arrs):
    return [rg["torch"].from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def solve_ragged(rg, clouds, inits, max_iteration):
    out = rg["R"].registration_icp_ragged(to_dev(rg, [c[0] for c in clouds]), to_dev(rg, [c[1] for c in clouds]), MD, inits,
                                          max_iteration=max_iteration)
    rg["torch"].cuda.synchronize()
    return out


def solve_alone(rg, cloud, init, max_iteration):
    s, t = to_dev(rg, cloud)
    return rg["R"].registration_icp(s, t, MD, init, max_iteration=max_iteration)


def assert_same_bits(got, exp, tag):
    for name, a, b in zip(("T", "fitness", "rmse", "iterations"), got, exp):
        assert np.array_equal(np.asarray(a), np.asarray(b)), (tag, name, a, b)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("max_iteration", [0, 1, 30])
def test_pairs_of_different_cell_budgets_in_one_launch(rg, max_iteration, mode):
    pairs = fused_pairs()
    nts = [nt for _, nt, _ in pairs]
    plan = ragged_plan(rg, nts)
    assert plan[:2] == (len(pairs), 0), plan
    assert plan[2] == max(R.plan(nt)[2] for nt in nts) and len({R.plan(nt)[1] for nt in nts}) >= 3
    assert any(nt % 4 == 1 and nt > 1 for nt in nts) and [k for _, _, k in pairs].count(0) == 1
    clouds, inits = make(pairs)
    with library_modes(rg, mode):
        got = solve_ragged(rg, clouds, inits, max_iteration)
        assert len(got) == len(pairs)
        for j, (ns, nt, k) in enumerate(pairs):
            tag = "pair %d (ns %d nt %d K %d) max_iteration %d mode %d" % (j, ns, nt, k, max_iteration, mode)
            assert got[j][0].shape == (k, 4, 4) and all(len(x) == k for x in got[j][1:]), tag
            if k == 0:
                continue
            assert_same_bits(got[j], solve_alone(rg, clouds[j], inits[j], max_iteration), tag)
            if max_iteration == 0:
                assert np.array_equal(got[j][0], inits[j]) and not got[j][3].any(), tag
            elif ns >= 257 and nt >= 1000:
                assert (got[j][3] >= 1).all() and (got[j][1] > 0).all(), tag       # (the solve did something)


@pytest.mark.parametrize("mode", [0, 1])
def test_the_same_pair_at_two_positions_gives_equal_bits(rg, mode):
    budgets, _ = R.path_sizes()
    pairs = [(700, 2001, 3), (300, budgets[0][1], 2), (700, 2001, 3), (50, 64, 1)]
    clouds, inits = make(pairs)
    clouds[2], inits[2] = clouds[0], inits[0]
    assert ragged_plan(rg, [p[1] for p in pairs])[:2] == (4, 0)
    with library_modes(rg, mode):
        got = solve_ragged(rg, clouds, inits, 30)
        again = solve_ragged(rg, clouds, inits, 30)
    assert_same_bits(got[0], got[2], "positions 0 and 2")
    for j in range(4):
        assert_same_bits(got[j], again[j], "two runs, pair %d" % j)
    assert (got[0][3] >= 1).all()


def test_a_single_init_returns_unbatched_values_and_packed_input_is_read(rg):
    pairs = [(300, 900, 1), (200, 400, 2)]
    clouds, inits = make(pairs)
    inits[0] = inits[0][0]
    torch = rg["torch"]
    src, tgt = to_dev(rg, [c[0] for c in clouds]), to_dev(rg, [c[1] for c in clouds])
    got = rg["R"].registration_icp_ragged((torch.cat(src), [0, 300, 500]), (torch.cat(tgt), torch.tensor([0, 900, 1300])), MD, inits)
    assert got[0][0].shape == (4, 4) and isinstance(got[0][1], float) and isinstance(got[0][3], int)
    assert_same_bits(got[0], solve_alone(rg, clouds[0], inits[0], 30), "pair 0")
    assert_same_bits(got[1], solve_alone(rg, clouds[1], inits[1], 30), "pair 1")
    with pytest.raises(ValueError, match="offsets of sources live on the host"):
        rg["R"].registration_icp_ragged((torch.cat(src), torch.tensor([0, 300, 500], device="cuda")), tgt, MD, inits)


@pytest.mark.parametrize("mode", [0, 1])
def test_a_call_that_also_holds_a_multi_launch_pair(rg, oracle, mode):
    budgets, first_loop = R.path_sizes()
    pairs = [(400, 1501, 3), (501, first_loop, 2), (63, budgets[2][1], 1)]
    assert R.plan(first_loop)[0] == 0 and R.plan(first_loop - 1)[0] == 1
    assert ragged_plan(rg, [p[1] for p in pairs])[:2] == (2, 1)
    clouds, inits = make(pairs, seed=3)
    with library_modes(rg, mode):
        got = solve_ragged(rg, clouds, inits, 30)
        for j in (0, 2):
            assert_same_bits(got[j], solve_alone(rg, clouds[j], inits[j], 30), "fused pair %d beside a loop pair, mode %d" % (j, mode))
    src, tgt = clouds[1]
    bar = 1e-6 * max(1.0, float(np.abs(tgt).max()))
    T, fit, rmse, its = got[1]
    for c in range(2):
        oT, ofit, ormse, oits = oracle.icp(src, tgt, MD, init=inits[1][c], fma_mode=mode)
        print("loop pair cand %d mode %d: fitness %.17g / %.17g its %d / %d  T %.2e  rmse %.2e"
              % (c, mode, fit[c], ofit, its[c], oits, np.abs(T[c] - oT).max(), abs(rmse[c] - ormse)))
        assert fit[c] == ofit and its[c] == oits, (c, fit[c], ofit, its[c], oits)
        np.testing.assert_allclose(T[c], oT, rtol=0, atol=bar)
        assert abs(rmse[c] - ormse) < 1e-7
        assert its[c] >= 1 and fit[c] > 0


def many_small_pairs(seed, s=257):
    """(sources, targets, candidates per pair) of s tiny pairs: 3 to 8 source points, 4 to 9 target points; pair 0, one in the
    middle and the last two without candidates, every seventh of the others with two, the rest with one."""
    rng = np.random.default_rng(seed)
    src = [rng.uniform(-0.1, 0.1, (int(rng.integers(3, 9)), 3)).astype(np.float32) for _ in range(s)]
    tgt = [rng.uniform(-0.1, 0.1, (int(rng.integers(4, 10)), 3)).astype(np.float32) for _ in range(s)]
    ks = [0 if j in (0, s // 2, s - 2, s - 1) else (2 if j % 7 == 3 else 1) for j in range(s)]
    return src, tgt, ks


def test_more_pairs_than_one_library_call_takes(rg):
    """257 pairs, one more than genpc_icp_batch_ragged takes: every pair's result is the bits of a one-pair call of the same
    function (both take the one-workgroup plan), and the pairs without candidates -- the first, one in the middle, the last of
    the first library call and the only one of the second -- come out empty."""
    s = 257
    assert s == rg["R"].ICP_RAGGED_MAX_PAIRS + 1
    src, tgt, ks = many_small_pairs(41, s)
    assert [j for j in range(s) if ks[j] == 0] == [0, 128, 255, 256] and ks.count(2) >= 3
    inits = [np.array(R.inits(900 + j, max(k, 1))[:k]).reshape(k, 4, 4) for j, k in enumerate(ks)]
    S_, T_ = to_dev(rg, src), to_dev(rg, tgt)
    got = rg["R"].registration_icp_ragged(S_, T_, MD, inits, max_iteration=2)
    assert len(got) == s
    for j in range(s):
        assert got[j][0].shape == (ks[j], 4, 4) and all(len(x) == ks[j] for x in got[j][1:]), j
        if ks[j] == 0:
            continue
        alone = rg["R"].registration_icp_ragged([S_[j]], [T_[j]], MD, [inits[j]], max_iteration=2)
        assert_same_bits(got[j], alone[0], "pair %d of %d" % (j, s))
    assert sum(int((g[1] > 0).sum()) for g in got) > s // 2          # (most solves found correspondences)
