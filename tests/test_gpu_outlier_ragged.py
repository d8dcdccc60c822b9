"""genpc_outlier_filter_ragged (csrc/knn.hip) on the GPU, all the clouds of outlier_cases.py in one call: the statistics against
outlier_cases.stats_ref of the oracle's means BIT FOR BIT (the summation order is part of the interface), the mask against
m < thr of those statistics and, on the finite clouds, against oracle.statistical_outlier_mask (test_outlier_ragged_host.py
checks on the CPU that these inputs keep every mean a relative 1e-9 away from its threshold); the counts; the optional
outputs; the clouds whose result IEEE arithmetic decides; and remove_noise_from_point_clouds against a loop of
remove_noise_from_point_cloud."""
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


def c_filter(km, names, k, ratio, mode, want_mean=True, want_stats=True, want_kept=True):
    """One call of the C entry point on the packed clouds; the outputs as numpy arrays (None where not asked for).  Every
    output starts filled with a sentinel no result can be."""
    torch, L = km["torch"], km["L"]
    off = oc.offsets(names)
    c, total = len(names), off[-1]
    P = torch.from_numpy(oc.packed(names)).cuda()
    mean = torch.full((total,), -7.0, device="cuda") if want_mean else None
    stats = torch.full((c, 3), -7.0, dtype=torch.float64, device="cuda") if want_stats else None
    keep = torch.full((total,), 9, dtype=torch.uint8, device="cuda")
    kept = torch.full((c,), -7, dtype=torch.int32, device="cuda") if want_kept else None
    arr = (ctypes.c_int * len(off))(*off)
    prev = km["lib"].genpc_set_arith(mode)
    try:
        rc = L.on_device_of(P, km["lib"].genpc_outlier_filter_ragged, c, ctypes.cast(arr, ctypes.c_void_p), L.ptr(P), k, float(ratio),
                            L.ptr(mean), L.ptr(stats), L.ptr(keep), L.ptr(kept))
    finally:
        km["lib"].genpc_set_arith(prev)
    assert rc == 1, L.last_error()
    host = lambda t: None if t is None else t.cpu().numpy()      # noqa: E731
    return dict(off=off, mean=host(mean), stats=host(stats), keep=host(keep), kept=host(kept))


_RUNS = {}


def full(km, k, ratio, mode):
    if (k, ratio, mode) not in _RUNS:
        _RUNS[(k, ratio, mode)] = c_filter(km, oc.ORDER, k, ratio, mode)
    return _RUNS[(k, ratio, mode)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("ratio", [1.5, 2.5])
@pytest.mark.parametrize("k", [8, 20])
def test_statistics_mask_and_counts(km, oracle, k, ratio, mode):
    r = full(km, k, ratio, mode)
    off = r["off"]
    assert set(np.unique(r["keep"]).tolist()) <= {0, 1}              # every byte written, with 0 or 1
    for j, name in enumerate(oc.ORDER):
        m = oc.oracle_means(oracle, name, k, mode)
        sl = slice(off[j], off[j + 1])
        np.testing.assert_array_equal(r["mean"][sl], m, err_msg=name)
        want = np.array(oc.stats_ref(m, ratio), np.float64)
        assert oc.same_bits(r["stats"][j], want), (name, r["stats"][j].tolist(), want.tolist())
        with np.errstate(invalid="ignore"):
            mask = m.astype(np.float64) < r["stats"][j, 2]
        np.testing.assert_array_equal(r["keep"][sl].astype(bool), mask, err_msg=name)
        assert r["kept"][j] == int(mask.sum()), name
        if name in oc.FINITE:
            np.testing.assert_array_equal(mask, oracle.statistical_outlier_mask(oc.CLOUDS[name], k, ratio, mode), err_msg=name)


@pytest.mark.parametrize("missing", ["mean", "stats", "kept", "all"])
def test_optional_outputs_may_be_null(km, missing):
    ref = full(km, 20, 1.5, 1)
    r = c_filter(km, oc.ORDER, 20, 1.5, 1, want_mean=missing not in ("mean", "all"), want_stats=missing not in ("stats", "all"),
                 want_kept=missing not in ("kept", "all"))
    assert r["keep"].tobytes() == ref["keep"].tobytes()
    for name in ("mean", "kept"):
        if r[name] is not None:
            assert r[name].tobytes() == ref[name].tobytes()
    if r["stats"] is not None:
        assert oc.same_bits(r["stats"], ref["stats"])


def test_the_clouds_ieee_arithmetic_decides(km, oracle):
    r = full(km, 20, 2.5, 1)
    off = r["off"]
    at = oc.ORDER.index

    def of(name):
        j = at(name)
        return r["stats"][j], r["keep"][off[j]:off[j + 1]], r["kept"][j]

    st, keep, kept = of("u1")                                        # std = 0 / 0
    assert st[0] == 0.0 and np.isnan(st[1]) and np.isnan(st[2]) and keep.tolist() == [0] and kept == 0
    st, keep, kept = of("identical300")                              # every mean 0: thr = 0, and 0 < 0 is false
    assert st.tolist() == [0.0, 0.0, 0.0] and not keep.any() and kept == 0
    for name in ("nan700", "inf700"):                                # a NaN mean: the cloud's mean, std and thr are NaN
        st, keep, kept = of(name)
        assert np.isnan(st).all() and keep.shape == (700,) and not keep.any() and kept == 0
    st, keep, kept = of("empty")
    assert np.isnan(st).all() and keep.shape == (0,) and kept == 0
    for name in ("nan700", "inf700", "empty"):                       # the clouds beside them have not noticed
        for nb in (oc.ORDER[at(name) - 1], oc.ORDER[at(name) + 1]):
            assert nb in oc.FINITE
            _, keep, kept = of(nb)
            want = oracle.statistical_outlier_mask(oc.CLOUDS[nb], 20, 2.5, 1)
            np.testing.assert_array_equal(keep.astype(bool), want, err_msg=nb)
            assert kept == int(want.sum()) and 0 < kept < want.shape[0] + 1


def test_the_order_of_the_batch_does_not_matter(km):
    fwd = full(km, 20, 1.5, 1)
    rev = c_filter(km, oc.ORDER[::-1], 20, 1.5, 1)
    assert oc.same_bits(fwd["stats"], rev["stats"][::-1])
    assert fwd["kept"].tolist() == rev["kept"][::-1].tolist()
    n = len(oc.ORDER)
    for j in range(n):
        a = fwd["keep"][fwd["off"][j]:fwd["off"][j + 1]]
        b = rev["keep"][rev["off"][n - 1 - j]:rev["off"][n - j]]
        assert a.tobytes() == b.tobytes(), oc.ORDER[j]


@pytest.mark.parametrize("ratio", [1.5, 2.5])
def test_remove_noise_from_point_clouds_equals_the_loop(km, ratio):
    torch, R = km["torch"], km["R"]
    clouds = [torch.from_numpy(oc.CLOUDS[n]).cuda() for n in oc.ORDER]
    filtered, keeps, stats, kept = R.remove_noise_from_point_clouds(clouds, nb_neighbors=20, std_ratio=ratio, return_stats=True)
    assert len(filtered) == len(keeps) == len(clouds)
    assert stats.dtype == torch.float64 and tuple(stats.shape) == (len(clouds), 3) and stats.is_cuda
    assert kept.dtype == torch.int32 and tuple(kept.shape) == (len(clouds),) and kept.is_cuda
    for name, c, f, k, n in zip(oc.ORDER, clouds, filtered, keeps, kept.tolist()):
        f1, k1 = R.remove_noise_from_point_cloud(c, nb_neighbors=20, std_ratio=ratio)
        assert k.dtype == torch.bool and torch.equal(k, k1), name
        assert torch.equal(f, f1) and f.shape[0] == n, name
    two = R.remove_noise_from_point_clouds(clouds, nb_neighbors=20, std_ratio=ratio)
    assert len(two) == 2 and all(torch.equal(a, b) for a, b in zip(two[0], filtered))


def test_more_than_384_clouds_take_several_calls(km):
    torch, R = km["torch"], km["R"]
    rng = np.random.default_rng(391)
    clouds = [torch.from_numpy(rng.random((30 + j % 7, 3), dtype=np.float32)).cuda() for j in range(391)]
    filtered, keeps, stats, kept = R.remove_noise_from_point_clouds(clouds, nb_neighbors=8, std_ratio=1.5, return_stats=True)
    assert len(filtered) == 391 and [f.shape[0] for f in filtered] == kept.tolist()
    for j in (0, 383, 384, 390):
        one = R.remove_noise_from_point_clouds([clouds[j]], nb_neighbors=8, std_ratio=1.5, return_stats=True)
        assert torch.equal(one[1][0], keeps[j]) and oc.same_bits(one[2].cpu().numpy(), stats[j].cpu().numpy())
