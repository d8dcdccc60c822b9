"""genpc_knn_mean_distance_ragged (csrc/knn.hip) on the GPU: all the clouds of outlier_cases.py in ONE call, every cloud's
slice against oracle.knn_mean_distance on that cloud alone, bit for bit and NaN for NaN, in both arithmetic modes; the batch in
reversed order; one cloud against the single call; 384 tiny clouds; two runs; what the C entry point refuses (nothing written);
and the calls that have nothing to do."""
import ctypes

import numpy as np
import pytest

import outlier_cases as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def km():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib, reg_xyz
    return dict(torch=torch, L=_lib, lib=_lib.lib, R=reg_xyz)


def run(km, names, k, mode, packed_form=False):
    """The means of the clouds `names`, one call, as a list of numpy arrays."""
    torch = km["torch"]
    prev = km["lib"].genpc_set_arith(mode)
    try:
        if packed_form:
            got = km["R"].knn_mean_distance_ragged((torch.from_numpy(oc.packed(names)).cuda(), oc.offsets(names)), k)
        else:
            got = km["R"].knn_mean_distance_ragged([torch.from_numpy(oc.CLOUDS[n]).cuda() for n in names], k)
        return [g.cpu().numpy() for g in got]
    finally:
        km["lib"].genpc_set_arith(prev)


_BATCH = {}


def batch(km, k, mode):
    if (k, mode) not in _BATCH:
        _BATCH[(k, mode)] = run(km, oc.ORDER, k, mode)
    return _BATCH[(k, mode)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("k", [8, 20])
def test_every_cloud_of_one_call_equals_the_oracle(km, oracle, k, mode):
    got = batch(km, k, mode)
    assert len(got) == len(oc.ORDER)
    for name, m in zip(oc.ORDER, got):
        assert m.dtype == np.float32 and m.shape == (oc.CLOUDS[name].shape[0],), name
        np.testing.assert_array_equal(m, oc.oracle_means(oracle, name, k, mode), err_msg=name)
    assert np.isnan(got[oc.ORDER.index("nan700")][317]) and np.isnan(got[oc.ORDER.index("inf700")][203])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("k", [16, 32])
def test_the_other_list_lengths(km, oracle, k, mode):
    names = ["lattice", "u8193"]
    for name, m in zip(names, run(km, names, k, mode)):
        np.testing.assert_array_equal(m, oc.oracle_means(oracle, name, k, mode), err_msg=name)


@pytest.mark.parametrize("mode", [0, 1])
def test_reversed_batch_and_packed_form_give_the_same_bits(km, mode):
    fwd = batch(km, 20, mode)
    rev = run(km, oc.ORDER[::-1], 20, mode, packed_form=True)[::-1]
    for name, a, b in zip(oc.ORDER, fwd, rev):
        assert a.tobytes() == b.tobytes(), name


@pytest.mark.parametrize("name", ["u1", "u257", "u8193", "lattice", "nan700"])
def test_one_cloud_equals_the_single_call(km, name):
    torch = km["torch"]
    P = torch.from_numpy(oc.CLOUDS[name]).cuda()
    for k in (8, 20):
        single = km["R"].knn_mean_distance(P, k).cpu().numpy()
        assert run(km, [name], k, km["lib"].genpc_get_arith())[0].tobytes() == single.tobytes()


def test_384_tiny_clouds(km, oracle):
    torch = km["torch"]
    rng = np.random.default_rng(384)
    clouds = [rng.random((1 + j % 40, 3), dtype=np.float32) for j in range(384)]
    got = km["R"].knn_mean_distance_ragged([torch.from_numpy(c).cuda() for c in clouds], 20)
    assert len(got) == 384
    mode = km["lib"].genpc_get_arith()
    for j, (c, g) in enumerate(zip(clouds, got)):
        np.testing.assert_array_equal(g.cpu().numpy(), oracle.knn_mean_distance(c, 20, mode), err_msg="cloud %d" % j)


def test_more_than_384_clouds_take_several_calls(km, oracle):
    torch = km["torch"]
    rng = np.random.default_rng(390)
    clouds = [rng.random((3 + j % 5, 3), dtype=np.float32) for j in range(390)]
    got = km["R"].knn_mean_distance_ragged([torch.from_numpy(c).cuda() for c in clouds], 8)
    mode = km["lib"].genpc_get_arith()
    for j in (0, 383, 384, 389):
        np.testing.assert_array_equal(got[j].cpu().numpy(), oracle.knn_mean_distance(clouds[j], 8, mode), err_msg="cloud %d" % j)


def test_two_runs_give_identical_bytes(km):
    a = run(km, oc.ORDER, 20, 1)
    b = batch(km, 20, 1)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_device_resident_offsets_raise(km):
    torch = km["torch"]
    with pytest.raises(ValueError, match="the offsets of clouds live on the host"):
        km["R"].knn_mean_distance_ragged((torch.zeros(8, 3).cuda(), torch.tensor([0, 3, 8], dtype=torch.int32).cuda()))


def c_call(km, c, off, xyz, k, out):
    arr = (ctypes.c_int * len(off))(*off) if off is not None else None
    return km["L"].on_device_of(out, km["lib"].genpc_knn_mean_distance_ragged, c, ctypes.cast(arr, ctypes.c_void_p) if arr is not None else None,
                                km["L"].ptr(xyz), k, km["L"].ptr(out))


REFUSALS = {
    "c = 385": lambda P: (385, [0] + [1] * 385, P, 20),
    "k = 7": lambda P: (2, [0, 30, 64], P, 7),
    "off[0] = 1": lambda P: (2, [1, 30, 64], P, 20),
    "a descending offset": lambda P: (3, [0, 40, 30, 64], P, 20),
    "a null xyz": lambda P: (2, [0, 30, 64], None, 20),
    "c = -1": lambda P: (-1, [0, 64], P, 20),
    "a null off": lambda P: (2, None, P, 20),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_the_entry_point_refuses_and_writes_nothing(km, case):
    torch = km["torch"]
    P = torch.from_numpy(oc.CLOUDS["u64"]).cuda()
    out = torch.full((64,), -7.0, device="cuda")
    c, off, xyz, k = REFUSALS[case](P)
    assert c_call(km, c, off, xyz, k, out) == -1
    assert "genpc_knn_mean_distance_ragged" in km["L"].last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    # the filter's entry point shares the checks
    keep = torch.full((64,), 9, dtype=torch.uint8, device="cuda")
    arr = (ctypes.c_int * len(off))(*off) if off is not None else None
    rc = km["L"].on_device_of(keep, km["lib"].genpc_outlier_filter_ragged, c, ctypes.cast(arr, ctypes.c_void_p) if arr is not None else None,
                              km["L"].ptr(xyz), k, 1.5, None, None, km["L"].ptr(keep), None)
    assert rc == -1 and "genpc_outlier_filter_ragged" in km["L"].last_error()
    torch.cuda.synchronize()
    assert bool((keep == 9).all())


def test_nothing_to_do_returns_1_and_writes_nothing(km):
    torch = km["torch"]
    P = torch.from_numpy(oc.CLOUDS["u64"]).cuda()
    out = torch.full((64,), -7.0, device="cuda")
    assert c_call(km, 0, [0], P, 20, out) == 1
    assert c_call(km, 0, None, P, 20, out) == 1
    assert c_call(km, 3, [0, 0, 0, 0], P, 20, out) == 1
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert [g.numel() for g in km["R"].knn_mean_distance_ragged([P[:0], P[:0]])] == [0, 0]
