"""The large farthest-point sampler (csrc/fps_large.hip: one workgroup per cloud, running minima, chunk maxima and cell table in
global memory) and the range it gives the public entry points: clouds of more than 262144 points.  Every sequence is compared
element by element with the oracle's in both arithmetic modes, and where the cloud is small enough for them with the sequence
fps_sampling returns through the two older kernels.  genpc_fps_large (fps_sampling_large) sends clouds of any size to the new
kernel, so the shapes here stay small: the oracle costs n k distance evaluations on the CPU."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MULTI_MAX = 262144          # fps_sampling takes one of the two older kernels up to here
LIMIT = 4194304


@pytest.fixture(scope="module")
def fg():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib, fps
    return dict(torch=torch, lib=_lib, L=_lib.lib, fps=fps)


_REF = {}


def ref(oracle, name, x, k, mode):
    """The oracle's sequence of a case, computed once."""
    key = (name, x.shape[0], k, mode)
    if key not in _REF:
        r = oracle.fps(x, k, mode)
        r.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def in_mode(fg, mode, fn):
    prev = fg["L"].genpc_set_arith(mode)
    try:
        return fn()
    finally:
        fg["L"].genpc_set_arith(prev)


def check_large(fg, oracle, cases, mode):
    """cases: (name, cloud, k).  One ragged call of fps_sampling_large; each sequence against the oracle and fps_sampling."""
    torch = fg["torch"]
    X = [torch.from_numpy(x).cuda() for _, x, _ in cases]
    got = in_mode(fg, mode, lambda: [g.cpu().numpy() for g in fg["fps"].fps_sampling_large(X, [k for _, _, k in cases])])
    for (name, x, k), g, Xg in zip(cases, got, X):
        assert g.shape == (k,) and g.dtype == np.int32 and g[0] == 0, name
        np.testing.assert_array_equal(g, ref(oracle, name, x, k, mode), err_msg=name + " (against the oracle)")
        if x.shape[0] <= MULTI_MAX:
            old = in_mode(fg, mode, lambda: fg["fps"].fps_sampling(Xg, k).cpu().numpy())
            np.testing.assert_array_equal(g, old, err_msg=name + " (against fps_sampling)")
    return got


def uniform(seed, n):
    return (np.random.default_rng(seed).random((n, 3), dtype=np.float32) - np.float32(0.5)).astype(np.float32)


@pytest.mark.parametrize("mode", [0, 1])
def test_sizes_round_the_wave_and_k_of_1_and_n(fg, oracle, mode):
    """n in {1, 2, 63, 64, 65, 1000} with k = 1 and k = n, twelve clouds in one call; k = n returns a permutation."""
    cases = []
    for n in (1, 2, 63, 64, 65, 1000):
        x = uniform(100 + n, n)
        cases += [("uniform %d k=1" % n, x, 1), ("uniform %d k=n" % n, x, n)]
    got = check_large(fg, oracle, cases, mode)
    for (name, x, k), g in zip(cases, got):
        if k == x.shape[0]:
            assert sorted(g.tolist()) == list(range(k)), name


def test_more_clouds_than_one_launch_takes(fg, oracle):
    """A launch takes 32 clouds: 35 small ones of different sizes are two launches and five groups of the check."""
    check_large(fg, oracle, [("many %d" % i, uniform(400 + i, 150 + 7 * i), 20 + i) for i in range(35)], 1)


@pytest.mark.parametrize("mode", [0, 1])
def test_one_ragged_call(fg, oracle, mode):
    cases = [("ragged %d" % n, uniform(200 + n, n), k) for n, k in ((777, 777), (5000, 2048), (24577, 3000))]
    check_large(fg, oracle, cases, mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_positions_beyond_16_bits(fg, oracle, mode):
    """70000 points: positions pass 65535, which the LDS kernel's 16-bit cell starts could not hold."""
    check_large(fg, oracle, [("uniform 70000", uniform(7, 70000), 1500)], mode)


def stress_cases():
    rng = np.random.default_rng(11)
    n, k = 30000, 2000
    base = rng.random((n // 5, 3), dtype=np.float32) - np.float32(0.5)
    plane = np.concatenate([rng.random((n, 2), dtype=np.float32), np.zeros((n, 1), np.float32)], 1)
    line = np.zeros((n, 3), np.float32)
    line[:, 0] = rng.random(n, dtype=np.float32)
    line[:, 1:] = np.float32([0.25, -0.5])
    u = rng.random((n, 3), dtype=np.float32) - np.float32(0.5)
    return [("lattice 12^3", (rng.integers(0, 12, size=(n, 3)) / 12.0 - 0.5).astype(np.float32), k),
            ("duplicates of n/5 points", base[rng.integers(0, n // 5, size=n)].copy(), k),
            ("one point 5000 times", np.ones((5000, 3), np.float32), 50),
            ("plane", plane, k), ("line", line, k),
            ("near 1000, a few ulps apart", (rng.random((n, 3), dtype=np.float32) * np.float32(0.01) + np.float32(1000.0)).astype(np.float32), k),
            ("scale 1e-3", (u * np.float32(1e-3)).astype(np.float32), k), ("scale 1e3", (u * np.float32(1e3)).astype(np.float32), k)]


@pytest.mark.parametrize("mode", [0, 1])
def test_inputs_that_stress_the_rules(fg, oracle, mode):
    """Exact ties by the thousand (the tie path), duplicates, one repeated point (the running maximum is 0 after the first
    sample), one layer and one row of cells, coordinates whose spacing is a few ulps, small and large scales."""
    check_large(fg, oracle, stress_cases(), mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_fps_sampling_beyond_262144_points(fg, oracle, mode):
    """The public entry on the first size the older kernels refuse (ValueError before the large sampler)."""
    torch = fg["torch"]
    x = uniform(5, 262145)
    got = in_mode(fg, mode, lambda: fg["fps"].fps_sampling(torch.from_numpy(x).cuda(), 1024).cpu().numpy())
    np.testing.assert_array_equal(got, ref(oracle, "uniform 262145", x, 1024, mode))


@pytest.mark.parametrize("mode", [0, 1])
def test_three_samplers_in_one_call(fg, oracle, mode):
    torch = fg["torch"]
    cases = [("mixed %d" % n, uniform(300 + n, n), k) for n, k in ((1000, 100), (300000, 512), (30000, 512))]
    got = in_mode(fg, mode, lambda: fg["fps"].fps_sampling_multi([torch.from_numpy(x).cuda() for _, x, _ in cases], [k for _, _, k in cases]))
    for (name, x, k), g in zip(cases, got):
        np.testing.assert_array_equal(g.cpu().numpy(), ref(oracle, name, x, k, mode), err_msg=name)
    plan = (ctypes.c_int * 8)()
    assert [fg["L"].genpc_fps_plan(n, 0, ctypes.cast(plan, ctypes.c_void_p)) and plan[0] for n in (1000, 300000, 30000)] == [0, 2, 1]


def test_fps_subsample_beyond_262144_points(fg):
    torch = fg["torch"]
    pts = torch.from_numpy(uniform(9, 262145))[None].cuda()
    sub = fg["fps"].fps_subsample(pts, 64)
    assert sub.shape == (1, 64, 3) and torch.equal(sub[0, 0], pts[0, 0])
    idx = fg["fps"].fps_sampling(pts, 64).long()
    assert torch.equal(sub[0], pts[0][idx[0]])


def test_refusals(fg):
    torch = fg["torch"]
    F = fg["fps"]
    too_many = torch.empty(LIMIT + 1, 3, device="cuda")
    with pytest.raises(ValueError, match=str(LIMIT)):
        F.fps_sampling(too_many, 16)
    with pytest.raises(ValueError, match=str(LIMIT)):
        F.fps_sampling_multi([too_many], [16])
    with pytest.raises(ValueError, match=str(LIMIT)):
        F.fps_sampling_large([too_many], [16])
    del too_many
    small = torch.rand(10, 3, device="cuda")
    with pytest.raises(ValueError):
        F.fps_sampling(small, 11)
    with pytest.raises(ValueError):
        F.fps_sampling_large([small], [11])
    with pytest.raises(ValueError):
        F.fps_sampling_large([small], [0])


def test_repeatable_and_alone_beside_another_stream(fg):
    """The same call twice returns equal tensors; beside a second stream that runs Chamfer distances at 16384 x 16384 the sequence
    is the quiet run's and nothing is counted as timed out -- the sampler has no hand-off that could."""
    torch = fg["torch"]
    F = fg["fps"]
    from genpc_amd.loss_functions import chamfer_3DDist
    g = torch.Generator(device="cuda")
    g.manual_seed(40)
    pts = torch.rand(40000, 3, device="cuda", generator=g)
    quiet = F.fps_sampling_large([pts], [2000])[0]
    again = F.fps_sampling_large([pts], [2000])[0]
    assert torch.equal(quiet, again)
    a = torch.rand(1, 16384, 3, device="cuda", generator=g)
    b = torch.rand(1, 16384, 3, device="cuda", generator=g)
    cd = chamfer_3DDist()
    cd(a, b)
    torch.cuda.synchronize()
    before = dict(F.stats)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(40):
            d1, _, _, _ = cd(a, b)
    busy = F.fps_sampling_large([pts], [2000])[0]
    still_running = not side.query()
    side.synchronize()
    torch.cuda.synchronize()
    print("chamfer loop still running when the sampling returned:", still_running)
    assert torch.equal(busy, quiet)
    assert F.stats["timed_out"] == before["timed_out"] and F.stats["failed_check"] == before["failed_check"], F.stats


def test_rounds_are_reported(fg):
    torch = fg["torch"]
    pts = [torch.from_numpy(uniform(50 + n, n)).cuda() for n in (3000, 50000)]
    fg["fps"].fps_sampling_large(pts, [500, 500])
    rounds = (ctypes.c_int * 2)()
    assert fg["lib"].on_device_of(pts[0], fg["L"].genpc_fps_stats, 2, ctypes.addressof(rounds)) == 1
    assert 0 < rounds[0] <= 500 and 0 < rounds[1] <= 500, list(rounds)
