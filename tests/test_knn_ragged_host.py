"""The host side of the ragged k-nearest-neighbour query, without a GPU: genpc_knn_query_ragged is declared with 9 arguments,
bound and exported and the ABI version stands; what knn.knn_query_ragged and dataUtils.linear_interpolation_clouds refuse,
exercised on CPU tensors and on a tensor made to answer is_cuda; and the calls that have nothing to do.  (The search's work
items are numbered by csrc/ragged_items.h and the pair table is csrc/ragged_table.h, both as they stand, which
test_uhd_ragged_host.py and test_nn_ragged_host.py run under the sanitizers; no new host-only header came with the query.)"""
import pytest
import torch

from test_abi import header_prototypes


@pytest.fixture(scope="module")
def K():
    from genpc_amd import build
    build.build(verbose=False)
    from genpc_amd import knn
    return knn


@pytest.fixture(scope="module")
def D(K):
    from genpc_amd.utils import dataUtils
    return dataUtils


def clouds(*sizes):
    return [torch.arange(n * 3, dtype=torch.float32).reshape(n, 3) for n in sizes]


def test_the_symbol_is_declared_bound_and_exported(K):
    from genpc_amd import _lib
    assert header_prototypes().get("genpc_knn_query_ragged") == 9
    assert len(_lib.SIGNATURES["genpc_knn_query_ragged"][1]) == 9
    assert getattr(_lib.lib, "genpc_knn_query_ragged") is not None


def test_abi_version_is_28_in_library_and_binding(K):          # (this addition kept 27; 28: genpc_hpr_plan)
    from genpc_amd import _lib
    assert _lib.ABI_VERSION == 28 and _lib.lib.genpc_abi_version() == 28


def test_cpu_tensors_raise(K, D):
    for call in (lambda: K.knn_query_ragged(clouds(3, 5), clouds(4, 2), 2),
                 lambda: K.knn_query_ragged((torch.zeros(8, 3), [0, 3, 8]), (torch.zeros(6, 3), [0, 4, 6]), 5),
                 lambda: K.knn_query_ragged((torch.zeros(8, 3), [0, 3, 8]), clouds(4, 2), 1),
                 lambda: D.linear_interpolation_clouds(clouds(4, 6), clouds(3, 5), k=2),
                 lambda: D.linear_interpolation_clouds([c.double() for c in clouds(5, 6)], [c.double() for c in clouds(3, 5)], k=5)):
        with pytest.raises(RuntimeError, match="GPU tensors only"):
            call()


@pytest.mark.parametrize("k", [0, 33, -1])
def test_k_outside_1_to_32_raises(K, k):
    with pytest.raises(ValueError, match="knn_query_ragged: k must be 1 .. 32, got %d" % k):
        K.knn_query_ragged(clouds(3, 5), clouds(4, 2), k)


def test_lists_of_different_length_raise(K, D):
    with pytest.raises(ValueError, match="knn_query_ragged: 2 queries against 1 targets"):
        K.knn_query_ragged(clouds(3, 5), clouds(4), 2)
    with pytest.raises(ValueError, match="knn_query_ragged: 1 queries against 2 targets"):
        K.knn_query_ragged((torch.zeros(8, 3), [0, 8]), (torch.zeros(6, 3), [0, 4, 6]), 2)
    with pytest.raises(ValueError, match="linear_interpolation_clouds: 2 clouds against 1 sets of new points"):
        D.linear_interpolation_clouds(clouds(3, 5), clouds(4), k=2)


def test_a_pair_with_queries_and_no_targets_raises(K):
    with pytest.raises(ValueError, match="knn_query_ragged: pair 1 has 5 queries and no targets"):
        K.knn_query_ragged(clouds(3, 5, 0), clouds(4, 0, 0), 2)
    with pytest.raises(ValueError, match="knn_query_ragged: pair 0 has 3 queries and no targets"):
        K.knn_query_ragged((torch.zeros(8, 3), [0, 3, 8]), (torch.zeros(6, 3), [0, 0, 6]), 2)


SIDES = [("queries", lambda K, c: K.knn_query_ragged(c, clouds(4, 2), 2)),
         ("targets", lambda K, c: K.knn_query_ragged(clouds(4, 2), c, 2))]


@pytest.mark.parametrize("name,call", SIDES, ids=[s[0] for s in SIDES])
def test_the_wrapper_refuses_and_names_the_offending_element(K, name, call):
    fn = "knn_query_ragged"
    with pytest.raises(ValueError, match=r"%s: %s\[1\] must be an \[N,3\] tensor" % (fn, name)):
        call(K, [torch.zeros(3, 3), torch.zeros(5, 2)])
    with pytest.raises(ValueError, match=r"%s: %s\[0\] must be an \[N,3\] tensor" % (fn, name)):
        call(K, [torch.zeros(2, 4, 3), torch.zeros(5, 3)])
    with pytest.raises(TypeError, match=r"%s: %s\[1\] must be torch.float32, got torch.float16" % (fn, name)):
        call(K, [torch.zeros(3, 3), torch.zeros(5, 3).half()])
    with pytest.raises(TypeError, match=r"%s: packed %s must be torch.float32, got torch.float16" % (fn, name)):
        call(K, (torch.zeros(8, 3).half(), [0, 3, 8]))
    with pytest.raises(ValueError, match=r"%s: packed %s must be \[T,3\]" % (fn, name)):
        call(K, (torch.zeros(8, 2), [0, 3, 8]))
    with pytest.raises(ValueError, match="offsets of %s must ascend from 0 to its 8 points" % name):
        call(K, (torch.zeros(8, 3), [0, 3, 7]))
    with pytest.raises(ValueError, match="offsets of %s must ascend from 0 to its 8 points" % name):
        call(K, (torch.zeros(8, 3), [0, 5, 3, 8]))
    with pytest.raises(TypeError, match="%s: %s is a list" % (fn, name)):
        call(K, torch.zeros(2, 8, 3))


@pytest.mark.parametrize("name,call", SIDES, ids=[s[0] for s in SIDES])
def test_the_wrapper_refuses_device_resident_offsets(K, name, call):
    """A device tensor of offsets would have to be read back.  Without a GPU the refusal is exercised on a tensor made to answer
    is_cuda: the check reads that attribute and nothing else of the tensor."""

    class DeviceOffsets(torch.Tensor):
        is_cuda = True

    off = torch.tensor([0, 3, 8], dtype=torch.int32).as_subclass(DeviceOffsets)
    with pytest.raises(ValueError, match="knn_query_ragged: the offsets of %s live on the host" % name):
        call(K, (torch.zeros(8, 3), off))


def test_linear_interpolation_clouds_refuses_and_names_the_pair(D):
    fn = "linear_interpolation_clouds"
    with pytest.raises(ValueError, match=r"%s: clouds\[1\] must be an \[N,3\] tensor" % fn):
        D.linear_interpolation_clouds([torch.zeros(3, 3), torch.zeros(5, 2)], clouds(4, 2))
    with pytest.raises(ValueError, match=r"%s: new_points\[0\] must be an \[N,3\] tensor" % fn):
        D.linear_interpolation_clouds(clouds(4, 2), [torch.zeros(2, 4, 3), torch.zeros(5, 3)])
    with pytest.raises(TypeError, match="%s: clouds and new_points are lists" % fn):
        D.linear_interpolation_clouds(torch.zeros(2, 8, 3), clouds(4, 2))
    with pytest.raises(RuntimeError, match=r"GPU tensors only \(got a cpu tensor for clouds\[0\]\)"):
        D.linear_interpolation_clouds(clouds(4, 6), clouds(3, 5))

    class OnDevice(torch.Tensor):          # passes for a GPU tensor until the size check, which comes before any use of it
        is_cuda = True

    gpu = lambda *sizes: [c.as_subclass(OnDevice) for c in clouds(*sizes)]      # noqa: E731
    with pytest.raises(ValueError, match="%s: k = 5 neighbours of cloud 1 of 4 points" % fn):
        D.linear_interpolation_clouds(gpu(7, 4, 9), gpu(3, 3, 3), k=5)
    with pytest.raises(ValueError, match="%s: k = 2 neighbours of cloud 0 of 1 points" % fn):
        D.linear_interpolation_clouds(gpu(1), gpu(0))


def test_empty_lists_give_empty_lists(K, D):
    assert K.knn_query_ragged([], [], 2) == []
    assert D.linear_interpolation_clouds([], []) == []
    pairs, (dist, idx) = K.knn_query_ragged((torch.zeros(0, 3), [0]), (torch.zeros(0, 3), [0]), 3)
    assert pairs == [] and dist.shape == (0, 3) and idx.shape == (0, 3) and idx.dtype == torch.int32
