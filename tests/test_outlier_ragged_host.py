"""The host side of the ragged statistical outlier filter, without a GPU: genpc_knn_mean_distance_ragged and
genpc_outlier_filter_ragged are declared, bound and exported and the ABI version stands; what the Python wrappers of
reg_xyz.py refuse; and the INPUT CONDITION of the GPU tests, checked on the CPU: on every finite cloud of outlier_cases.py the
mask made from the statistics in the library's summation order (outlier_cases.stats_ref) is the oracle's mask, whose sums run
in numpy's order, and no mean lies within a relative 1e-9 of the threshold.  That is a condition on the inputs, not a
tolerance: measured on this generator the smallest margin is 5.7e-6 and the two orders move the threshold by at most 3e-16
relative.  (The work items of the search are numbered by csrc/ragged_items.h as it stands, which
test_uhd_ragged_host.py runs under the sanitizers; no new host-only header came with the filter.)"""
import numpy as np
import pytest
import torch

import outlier_cases as oc
from test_abi import header_prototypes


@pytest.fixture(scope="module")
def R():
    from genpc_amd import build
    build.build(verbose=False)
    from genpc_amd import reg_xyz
    return reg_xyz


def clouds(*sizes):
    return [torch.arange(n * 3, dtype=torch.float32).reshape(n, 3) for n in sizes]


def test_both_symbols_are_declared_bound_and_exported(R):
    from genpc_amd import _lib
    protos = header_prototypes()
    for name, nargs in (("genpc_knn_mean_distance_ragged", 6), ("genpc_outlier_filter_ragged", 10)):
        assert protos.get(name) == nargs
        assert len(_lib.SIGNATURES[name][1]) == nargs
        assert getattr(_lib.lib, name) is not None


def test_abi_version_is_28_in_library_and_binding(R):          # (this addition kept 27; 28: genpc_hpr_plan)
    from genpc_amd import _lib
    assert _lib.ABI_VERSION == 28 and _lib.lib.genpc_abi_version() == 28


def test_cpu_tensors_raise(R):
    for call in (lambda: R.knn_mean_distance_ragged(clouds(3, 5)),
                 lambda: R.knn_mean_distance_ragged((torch.zeros(8, 3), [0, 3, 8]), k=8),
                 lambda: R.remove_noise_from_point_clouds(clouds(30, 5)),
                 lambda: R.remove_noise_from_point_clouds((torch.zeros(8, 3), [0, 3, 8]), return_stats=True),
                 lambda: R.fuse_scans(clouds(3, 5), clouds(4, 2)),
                 lambda: R.fuse_scans(clouds(3, 5), clouds(4, 2), source_cols=clouds(3, 5), target_cols=clouds(4, 2))):
        with pytest.raises(RuntimeError, match="GPU tensors only"):
            call()


WRAPPERS = [("knn_mean_distance_ragged", lambda R, c: R.knn_mean_distance_ragged(c)),
            ("remove_noise_from_point_clouds", lambda R, c: R.remove_noise_from_point_clouds(c)),
            ("fuse_scans", lambda R, c: R.fuse_scans(c, clouds(4, 2)))]


@pytest.mark.parametrize("fn,call", WRAPPERS, ids=[w[0] for w in WRAPPERS])
def test_wrappers_refuse_and_name_the_offending_element(R, fn, call):
    name = "sources" if fn == "fuse_scans" else "clouds"
    with pytest.raises(ValueError, match=r"%s: %s\[1\] must be an \[N,3\] tensor" % (fn, name)):
        call(R, [torch.zeros(3, 3), torch.zeros(5, 2)])
    with pytest.raises(ValueError, match=r"%s: %s\[0\] must be an \[N,3\] tensor" % (fn, name)):
        call(R, [torch.zeros(2, 4, 3), torch.zeros(5, 3)])
    with pytest.raises(TypeError, match=r"%s: %s\[1\] must be torch.float32, got torch.float16" % (fn, name)):
        call(R, [torch.zeros(3, 3), torch.zeros(5, 3).half()])
    with pytest.raises(TypeError, match=r"%s: packed %s must be torch.float32, got torch.float16" % (fn, name)):
        call(R, (torch.zeros(8, 3).half(), [0, 3, 8]))
    with pytest.raises(ValueError, match=r"%s: packed %s must be \[T,3\]" % (fn, name)):
        call(R, (torch.zeros(8, 2), [0, 3, 8]))
    with pytest.raises(ValueError, match="offsets of %s must ascend from 0 to its 8 points" % name):
        call(R, (torch.zeros(8, 3), [0, 3, 7]))
    with pytest.raises(ValueError, match="offsets of %s must ascend from 0 to its 8 points" % name):
        call(R, (torch.zeros(8, 3), [0, 5, 3, 8]))
    with pytest.raises(TypeError, match="%s: %s is a list" % (fn, name)):
        call(R, torch.zeros(2, 8, 3))


@pytest.mark.parametrize("fn,call", WRAPPERS, ids=[w[0] for w in WRAPPERS])
def test_wrappers_refuse_device_resident_offsets(R, fn, call):
    """A device tensor of offsets would have to be read back.  Without a GPU the refusal is exercised on a `meta` tensor made
    to answer is_cuda: the check reads that attribute and nothing else of the tensor."""
    name = "sources" if fn == "fuse_scans" else "clouds"

    class DeviceOffsets(torch.Tensor):
        is_cuda = True

    off = torch.tensor([0, 3, 8], dtype=torch.int32).as_subclass(DeviceOffsets)
    with pytest.raises(ValueError, match="%s: the offsets of %s live on the host" % (fn, name)):
        call(R, (torch.zeros(8, 3), off))


def test_a_bad_k_and_mismatched_lists_raise(R):
    with pytest.raises(ValueError, match="k must be 8, 16, 20 or 32"):
        R.knn_mean_distance_ragged(clouds(3, 5), k=7)
    with pytest.raises(ValueError, match="nb_neighbors must be 8, 16, 20 or 32"):
        R.remove_noise_from_point_clouds(clouds(3, 5), nb_neighbors=5)
    with pytest.raises(ValueError, match="2 sources against 1 targets"):
        R.fuse_scans(clouds(3, 5), clouds(4))
    assert R.knn_mean_distance_ragged([]) == [] and R.fuse_scans([], []) == []


def test_stats_ref_is_the_defined_order():
    """The restated order against a literal transcription of the definition on a size that has a ragged last row."""
    rng = np.random.default_rng(5)
    v = rng.standard_normal(2500)
    p = [0.0] * 1024
    for i in range(2500):
        p[i % 1024] = p[i % 1024] + float(v[i])
    w = 512
    while w >= 1:
        for t in range(w):
            p[t] = p[t] + p[t + w]
        w //= 2
    assert oc.ordered_sum(v) == p[0]
    assert np.isnan(oc.stats_ref(np.zeros(0, np.float32), 1.5)).all()
    mean, std, thr = oc.stats_ref(np.array([0.25], np.float32), 1.5)
    assert mean == 0.25 and np.isnan(std) and np.isnan(thr)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("k", [8, 20])
def test_the_input_condition(oracle, k, mode):
    margins = {}
    for name in oc.FINITE:
        P = oc.CLOUDS[name]
        m = oc.oracle_means(oracle, name, k, mode)
        assert np.isfinite(m).all(), name
        for ratio in (1.5, 2.5):
            np.testing.assert_array_equal(oc.mask_ref(m, ratio), oracle.statistical_outlier_mask(P, k, ratio, mode), err_msg="%s %g" % (name, ratio))
            g = oc.margin(m, oc.stats_ref(m, ratio)[2])
            if g is not None:
                margins[(name, ratio)] = g
    print("k=%d mode=%d smallest margin %.3g at %s" % (k, mode, min(margins.values()), min(margins, key=margins.get)))
    assert len(margins) >= 2 * (len(oc.FINITE) - 2)             # (u1: thr is NaN; identical300: thr is 0)
    assert all(g > 1e-9 for g in margins.values()), sorted(margins.items(), key=lambda kv: kv[1])[:3]
