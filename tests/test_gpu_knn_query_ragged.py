"""genpc_knn_query_ragged (csrc/knn_query.hip) on the GPU: the cases of test_gpu_knn_query.py as the pairs of ONE call.

Every pair's rows against the numpy brute force (mode 0) and against genpc_knn_query on that pair alone (modes 0 and 1), bit
for bit, distances and indices -- the key order distance bits << 32 | index makes ties exact, so there is no tolerance anywhere;
the pairs reversed and shuffled; one pair against the rectangular call; mode 1 against exact rationals on the tiny inputs;
385 pairs through the wrapper; what the C entry point writes, refuses and copies; two runs and a second stream; and
dataUtils.linear_interpolation_clouds against the recording of the reference's linear_interpolation."""
import ctypes

import numpy as np
import pytest

from test_gpu_knn_query import CASES, TINY, _tiny_inputs
from test_knn_reference_vectors import knn_bruteforce, select_k, sqdist_fma_exact

pytestmark = pytest.mark.gpu

KS = [1, 5, 8, 20, 32]


def _pairs():
    P = [(n,) + CASES[n][:2] for n in ("nt1", "nt3_k5", "identical", "lattice", "dup10", "far_outside", "offset_1e3", "nq1", "nq63",
                                      "nq65", "nq257")]
    q3, t3, _ = CASES["batch3"]
    P += [("batch3_%d" % e, q3[e], t3[e]) for e in range(3)]
    P.append(("nonfinite_targets",) + CASES["nonfinite_targets"][:2])
    none = np.zeros((0, 3), np.float32)
    P.append(("q0_t0", none, none))
    P.append(("q0_t40", none, np.random.default_rng(40).random((40, 3), dtype=np.float32)))
    return [(n, np.ascontiguousarray(q, np.float32), np.ascontiguousarray(t, np.float32)) for n, q, t in P]


PAIRS = _pairs()
_REF = {}


def brute(name, q, t, k):
    """Mode 0 brute force of a pair, computed once per (pair, k) and shared."""
    if (name, k) not in _REF:
        _REF[(name, k)] = knn_bruteforce(q, t, k) if len(q) else (np.zeros((0, k), np.float32), np.zeros((0, k), np.int32))
    return _REF[(name, k)]


@pytest.fixture(scope="module")
def kr():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib
    from genpc_amd.knn import knn_query, knn_query_ragged
    from genpc_amd.utils import dataUtils
    return dict(torch=torch, L=_lib, lib=_lib.lib, knn=knn_query, ragged=knn_query_ragged, D=dataUtils)


def offsets(clouds):
    return [0] + [int(v) for v in np.cumsum([len(c) for c in clouds])]


def run(kr, pairs, k, mode, packed_form=False):
    """One knn_query_ragged call on `pairs` [(name, q, t)]: a list of (dist, idx) numpy arrays."""
    torch = kr["torch"]
    prev = kr["lib"].genpc_set_arith(mode)
    try:
        qs, ts = [p[1] for p in pairs], [p[2] for p in pairs]
        if packed_form:
            got, (pd, pi) = kr["ragged"]((torch.from_numpy(np.concatenate(qs)).cuda(), offsets(qs)),
                                         (torch.from_numpy(np.concatenate(ts)).cuda(), offsets(ts)), k)
            assert pd.shape == (sum(len(q) for q in qs), k) and pi.shape == pd.shape
        else:
            got = kr["ragged"]([torch.from_numpy(q).cuda() for q in qs], [torch.from_numpy(t).cuda() for t in ts], k)
        torch.cuda.synchronize()
        return [(d.cpu().numpy(), i.cpu().numpy()) for d, i in got]
    finally:
        kr["lib"].genpc_set_arith(prev)


def single(kr, q, t, k, mode):
    torch = kr["torch"]
    prev = kr["lib"].genpc_set_arith(mode)
    try:
        d, i = kr["knn"](torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda(), k)
        torch.cuda.synchronize()
        return d.cpu().numpy(), i.cpu().numpy()
    finally:
        kr["lib"].genpc_set_arith(prev)


_BATCH = {}


def batch(kr, k, mode):
    if (k, mode) not in _BATCH:
        _BATCH[(k, mode)] = run(kr, PAIRS, k, mode)
    return _BATCH[(k, mode)]


def assert_same(got, want, what):
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32 and got[0].shape == want[0].shape == got[1].shape, what + ": shape"
    np.testing.assert_array_equal(got[1], want[1], err_msg=what + ": indices")
    assert got[0].tobytes() == want[0].tobytes(), what + ": distance bits"


@pytest.mark.parametrize("k", KS)
def test_mode0_every_pair_is_the_brute_force_bit_for_bit(kr, k):
    got = batch(kr, k, 0)
    assert len(got) == len(PAIRS)
    for (name, q, t), g in zip(PAIRS, got):
        assert g[0].shape == (len(q), k), name
        assert_same(g, brute(name, q, t, k), "%s k=%d" % (name, k))
        if len(q) and len(t) < k:
            assert (g[1][:, len(t):] == -1).all() and np.isposinf(g[0][:, len(t):]).all(), name
    g = got[[p[0] for p in PAIRS].index("nonfinite_targets")]
    assert not np.isin(g[1], [17, 203]).any()
    assert (g[1][64:] == -1).all() and np.isposinf(g[0][64:]).all()               # non-finite queries list nothing


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("k", KS)
def test_every_pair_is_the_single_call_on_that_pair_alone(kr, k, mode):
    for (name, q, t), g in zip(PAIRS, batch(kr, k, mode)):
        if len(q) == 0:
            assert g[0].shape == (0, k) and g[1].shape == (0, k), name
            continue
        assert_same(g, single(kr, q, t, k, mode), "%s k=%d mode %d" % (name, k, mode))


@pytest.mark.parametrize("mode", [0, 1])
def test_reversed_and_shuffled_batches_give_every_pair_the_same_bytes(kr, mode):
    fwd = batch(kr, 5, mode)
    perm = [int(v) for v in np.random.default_rng(17).permutation(len(PAIRS))]
    for order, packed_form in ((list(range(len(PAIRS)))[::-1], True), (perm, False)):
        got = run(kr, [PAIRS[j] for j in order], 5, mode, packed_form)
        for at, j in enumerate(order):
            assert got[at][0].tobytes() == fwd[j][0].tobytes() and got[at][1].tobytes() == fwd[j][1].tobytes(), PAIRS[j][0]


@pytest.mark.parametrize("k", [5, 20])
@pytest.mark.parametrize("name", ["nq257", "lattice", "nonfinite_targets"])
def test_one_pair_equals_the_rectangular_call(kr, name, k):
    p = PAIRS[[p[0] for p in PAIRS].index(name)]
    mode = kr["lib"].genpc_get_arith()
    assert_same(run(kr, [p], k, mode)[0], single(kr, p[1], p[2], k, mode), "%s k=%d" % (name, k))


_EXACT = {}


@pytest.mark.parametrize("k", [1, 2, 5, 8])
def test_mode1_tiny_cases_in_one_batch_exact_rationals(kr, k):
    pairs = []
    for name in TINY:
        q, t = _tiny_inputs(name)
        assert len(q) <= 64 and len(t) <= 64
        if name not in _EXACT:
            _EXACT[name] = sqdist_fma_exact(q, t)
        pairs.append((name, np.ascontiguousarray(q), np.ascontiguousarray(t)))
    for (name, _, _), g in zip(pairs, run(kr, pairs, k, 1)):
        assert_same(g, select_k(_EXACT[name], k), "%s k=%d mode 1" % (name, k))


def test_385_pairs_take_two_library_calls(kr):
    rng = np.random.default_rng(385)
    pairs = [("p%d" % j, rng.random((3, 3), dtype=np.float32), rng.random((4, 3), dtype=np.float32)) for j in range(385)]
    got = run(kr, pairs, 3, 0)
    assert len(got) == 385
    for (name, q, t), g in zip(pairs, got):
        assert_same(g, knn_bruteforce(q, t, 3), name)


SENT_D, SENT_I = -7.0, -7            # a squared distance is never negative, an index never below -1


def c_args(kr, pairs):
    torch = kr["torch"]
    qs, ts = [p[1] for p in pairs], [p[2] for p in pairs]
    Q = torch.from_numpy(np.concatenate(qs)).cuda()
    T = torch.from_numpy(np.concatenate(ts)).cuda()
    return offsets(qs), Q, offsets(ts), T


def c_call(kr, c, noff, Q, moff, T, k, dist, idx):
    """The C entry point on torch's current stream; noff / moff: lists (copied to ctypes arrays), ctypes arrays, or None."""
    def arr(off):
        if off is None:
            return None
        a = off if isinstance(off, ctypes.Array) else (ctypes.c_int * len(off))(*off)
        return ctypes.cast(a, ctypes.c_void_p)
    p = kr["L"].ptr
    return kr["lib"].genpc_knn_query_ragged(c, arr(noff), p(Q), arr(moff), p(T), k, p(dist), p(idx),
                                            ctypes.c_void_p(kr["torch"].cuda.current_stream().cuda_stream))


def sentinels(kr, rows, k):
    torch = kr["torch"]
    return torch.full((rows, k), SENT_D, device="cuda"), torch.full((rows, k), SENT_I, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("k", [1, 5, 32])
def test_every_word_of_a_pair_with_queries_is_written_and_none_beyond(kr, k):
    torch = kr["torch"]
    noff, Q, moff, T = c_args(kr, PAIRS)
    dist, idx = sentinels(kr, noff[-1] + 16, k)                  # 16 rows of guard behind the call's own
    assert c_call(kr, len(PAIRS), noff, Q, moff, T, k, dist, idx) == 1
    torch.cuda.synchronize()
    assert not bool((dist[:noff[-1]] == SENT_D).any()) and not bool((idx[:noff[-1]] == SENT_I).any())
    assert bool((dist[noff[-1]:] == SENT_D).all()) and bool((idx[noff[-1]:] == SENT_I).all())
    mode = kr["lib"].genpc_get_arith()
    want = batch(kr, k, mode)
    assert dist[:noff[-1]].cpu().numpy().tobytes() == np.concatenate([w[0] for w in want]).tobytes()
    assert idx[:noff[-1]].cpu().numpy().tobytes() == np.concatenate([w[1] for w in want]).tobytes()


REFUSALS = {
    "k = 0": lambda a: dict(k=0),
    "k = 33": lambda a: dict(k=33),
    "a null noff": lambda a: dict(noff=None),
    "a null moff": lambda a: dict(moff=None),
    "noff[0] = 1": lambda a: dict(noff=[1] + a["noff"][1:]),
    "descending offsets": lambda a: dict(noff=[0, 9, 5] + a["noff"][3:]),
    "queries and no targets": lambda a: dict(moff=[0, 0] + a["moff"][2:]),
    "a null dist": lambda a: dict(dist=None),
    "a null idx": lambda a: dict(idx=None),
    "a null xyz2": lambda a: dict(T=None),
    "c = -1": lambda a: dict(c=-1),
    "c = 385": lambda a: dict(c=385, noff=[0] + [1] * 385, moff=[0] + [1] * 385),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_the_entry_point_refuses_and_writes_nothing(kr, case):
    torch = kr["torch"]
    pairs = PAIRS[:4]
    noff, Q, moff, T = c_args(kr, pairs)
    dist, idx = sentinels(kr, max(noff[-1], 385), 5)
    a = dict(c=len(pairs), noff=noff, Q=Q, moff=moff, T=T, k=5, dist=dist, idx=idx)
    a.update(REFUSALS[case](a))
    assert c_call(kr, a["c"], a["noff"], a["Q"], a["moff"], a["T"], a["k"], a["dist"], a["idx"]) == -1
    assert "genpc_knn_query_ragged" in kr["L"].last_error()
    torch.cuda.synchronize()
    assert bool((dist == SENT_D).all()) and bool((idx == SENT_I).all())


def test_nothing_to_do_returns_1_and_writes_nothing(kr):
    torch = kr["torch"]
    noff, Q, moff, T = c_args(kr, PAIRS[:4])
    dist, idx = sentinels(kr, noff[-1], 5)
    assert c_call(kr, 0, [0], Q, [0], T, 5, dist, idx) == 1
    assert c_call(kr, 0, None, Q, None, T, 5, dist, idx) == 1
    assert c_call(kr, 3, [0, 0, 0, 0], Q, [0, 5, 5, 9], T, 5, dist, idx) == 1
    assert c_call(kr, 2, [0, 0, 0], None, [0, 0, 0], None, 5, None, None) == 1
    assert c_call(kr, 3, [0, 0, 0, 0], Q, [0, 5, 3, 9], T, 5, dist, idx) == -1          # the offsets are checked first
    torch.cuda.synchronize()
    assert bool((dist == SENT_D).all()) and bool((idx == SENT_I).all())
    got = kr["ragged"]([Q[:0], Q[:0]], [T[:0], T[:7]], 5)
    assert [tuple(d.shape) for d, _ in got] == [(0, 5), (0, 5)]


def test_the_offsets_are_copied_before_the_call_returns(kr):
    torch = kr["torch"]
    noff, Q, moff, T = c_args(kr, PAIRS)
    mode = kr["lib"].genpc_get_arith()
    want = batch(kr, 8, mode)
    na, ma = (ctypes.c_int * len(noff))(*noff), (ctypes.c_int * len(moff))(*moff)
    dist, idx = sentinels(kr, noff[-1], 8)
    torch.cuda.synchronize()
    assert c_call(kr, len(PAIRS), na, Q, ma, T, 8, dist, idx) == 1
    for i in range(len(noff)):                                   # garbage, before anything is waited for
        na[i] = -123456789 + i
        ma[i] = 0x7fffffff - i
    torch.cuda.synchronize()
    assert dist.cpu().numpy().tobytes() == np.concatenate([w[0] for w in want]).tobytes()
    assert idx.cpu().numpy().tobytes() == np.concatenate([w[1] for w in want]).tobytes()


@pytest.mark.parametrize("mode", [0, 1])
def test_two_runs_and_a_second_stream_give_identical_bytes(kr, mode):
    torch = kr["torch"]
    a = batch(kr, 20, mode)
    b = run(kr, PAIRS, 20, mode)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = run(kr, PAIRS, 20, mode)
    s.synchronize()
    for (name, _, _), x, y, z in zip(PAIRS, a, b, c):
        assert x[0].tobytes() == y[0].tobytes() == z[0].tobytes() and x[1].tobytes() == y[1].tobytes() == z[1].tobytes(), name


@pytest.mark.parametrize("k", [2, 5])
def test_linear_interpolation_clouds_is_the_references(kr, golden, k):
    torch, D = kr["torch"], kr["D"]
    fx = golden("ref_py_interp.npz")
    by = {p[0]: p for p in PAIRS}
    clouds = [torch.from_numpy(by["batch3_2"][2]).cuda(), torch.from_numpy(fx["interp_points"]).cuda(), torch.from_numpy(by["nq257"][2]).cuda()]
    news = [torch.from_numpy(by["batch3_2"][1]).cuda(), torch.from_numpy(fx["interp_queries"]).cuda(), torch.from_numpy(by["nq257"][1]).cuda()]
    assert clouds[1].shape == (2048, 3) and news[1].shape == (1000, 3)
    got = kr["ragged"]([n.float() for n in news], clouds, k)
    np.testing.assert_array_equal(got[1][1].cpu().numpy(), fx["interp_idx6"][:, :k])
    out = D.linear_interpolation_clouds(clouds, news, k=k)
    assert len(out) == 3 and all(o.is_cuda and o.dtype == torch.float64 and o.shape == n.shape for o, n in zip(out, news))
    np.testing.assert_allclose(out[1].cpu().numpy(), fx["interp_k%d" % k], rtol=1e-9, atol=1e-12)
    for j in range(3):
        alone = D.linear_interpolation(clouds[j], news[j], k=k)
        np.testing.assert_allclose(out[j].cpu().numpy(), alone.cpu().numpy(), rtol=1e-9, atol=1e-12, err_msg="pair %d" % j)


def test_linear_interpolation_clouds_names_the_pair_without_k_finite_neighbours(kr):
    torch, D = kr["torch"], kr["D"]
    by = {p[0]: p for p in PAIRS}
    bad = by["nonfinite_targets"]                                # its last two queries are non-finite
    clouds = [torch.from_numpy(by["nq65"][2]).cuda(), torch.from_numpy(bad[2]).cuda()]
    news = [torch.from_numpy(by["nq65"][1]).cuda(), torch.from_numpy(bad[1]).cuda()]
    with pytest.raises(ValueError, match="linear_interpolation_clouds: pair 1 has a point without k neighbours"):
        D.linear_interpolation_clouds(clouds, news, k=2)
    with pytest.raises(ValueError, match="k = 5 neighbours of cloud 0 of 3 points"):
        D.linear_interpolation_clouds([clouds[0][:3], clouds[1]], news, k=5)
