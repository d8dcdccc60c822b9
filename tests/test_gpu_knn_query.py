"""genpc_knn_query (csrc/knn_query.hip) on the GPU.

Mode 0: distances AND indices equal a numpy brute force -- ((dx*dx + dy*dy) + dz*dz) in float32, ordered by the 64-bit key
distance bits << 32 | index -- bit for bit, on the smallest shapes at which the search can go wrong.  Mode 1: exact
rational emulation of the fused arithmetic on the tiny cases; on the large ones column 0 against nm_distance and the
oracle's chamfer_forward, and a self-query with k = 20 against oracle.knn_mean_distance."""
import numpy as np
import pytest

from test_knn_reference_vectors import knn_bruteforce, select_k, sqdist_fma_exact

pytestmark = pytest.mark.gpu

KS = [1, 2, 5, 8, 20, 32]


@pytest.fixture(scope="module")
def kq():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib, chamfer_3D
    from genpc_amd.knn import knn_query
    return dict(torch=torch, lib=_lib.lib, knn=knn_query, ch=chamfer_3D)


def hip_knn(kq, q, t, k, mode):
    torch = kq["torch"]
    prev = kq["lib"].genpc_set_arith(mode)
    try:
        d, i = kq["knn"](torch.from_numpy(np.ascontiguousarray(q)).cuda(), torch.from_numpy(np.ascontiguousarray(t)).cuda(), k)
        torch.cuda.synchronize()
    finally:
        kq["lib"].genpc_set_arith(prev)
    return d.cpu().numpy(), i.cpu().numpy()


def lattice():
    g = np.arange(8, dtype=np.float32) / np.float32(8)
    t = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(21)
    on = t[rng.choice(512, 40, replace=False)]
    wall = t[rng.choice(512, 60, replace=False)].copy()
    wall[:20, 0] += np.float32(1 / 16)                       # midway between 2 lattice points
    wall[20:40, :2] += np.float32(1 / 16)                    # between 4
    wall[40:] += np.float32(1 / 16)                          # between 8 (some of them outside the lattice's box)
    return np.concatenate([on, wall]), t


def clustered(seed, n):
    rng = np.random.default_rng(seed)
    c = rng.random((5, 3)) - 0.5
    return (c[rng.integers(0, 5, n)] + 0.02 * rng.normal(size=(n, 3))).astype(np.float32)


def _cases():
    rng = np.random.default_rng(20261017)
    u = lambda *s: rng.random(s, dtype=np.float32) - np.float32(0.5)      # noqa: E731
    c = {}
    c["nt1"] = (u(5, 3), u(1, 3), [1, 5])
    c["nt3_k5"] = (u(9, 3), u(3, 3), [5])
    same = np.repeat(u(1, 3), 40, axis=0)
    c["identical"] = (np.concatenate([same[:1], u(6, 3)]), same, [1, 8, 20])
    c["lattice"] = lattice() + (KS,)
    t = u(300, 3)
    t[100:110] = t[0:10]
    c["dup10"] = (np.concatenate([u(65, 3), t[0:10], t[0:10] + np.float32(1e-3)]), t, [1, 2, 5])
    far = np.concatenate([u(20, 3) + np.float32(50), u(20, 3) - np.float32(1000), u(23, 3) * np.float32(8)])
    c["far_outside"] = (far, u(500, 3), [5])
    c["offset_1e3"] = (u(65, 3) + np.float32(1e3), u(700, 3) + np.float32(1e3), [8])
    c["scale_1e-2"] = (u(65, 3) * np.float32(1e-2), u(700, 3) * np.float32(1e-2), [5])
    c["scale_1e2"] = (u(65, 3) * np.float32(1e2), u(700, 3) * np.float32(1e2), [5])
    t = u(700, 3)
    for nq in (1, 63, 65, 257):
        c["nq%d" % nq] = (u(nq, 3), t, [5])
    c["batch3"] = (np.stack([u(65, 3), u(65, 3) * np.float32(3), clustered(4, 65)]),
                   np.stack([u(300, 3), u(300, 3) * np.float32(2) + np.float32(1), clustered(5, 300)]), [8])
    c["clustered5000"] = (np.concatenate([clustered(7, 200), u(57, 3)]), clustered(6, 5000), KS)
    t = u(300, 3)
    t[17, 1] = np.nan
    t[203, 0] = np.inf
    c["nonfinite_targets"] = (np.concatenate([u(64, 3), t[17:18], t[203:204]]), t, [5])
    return c


CASES = _cases()
_REF = {}


def reference(name, k, mode):
    """Brute force of a case, computed once per (case, k, mode) and shared."""
    key = (name, k, mode)
    if key not in _REF:
        q, t, _ = CASES[name]
        qb, tb = (q, t) if q.ndim == 3 else (q[None], t[None])
        outs = []
        for e in range(qb.shape[0]):
            outs.append(knn_bruteforce(qb[e], tb[e], k) if mode == 0 else select_k(sqdist_fma_exact(qb[e], tb[e]), k))
        d, i = np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
        _REF[key] = (d, i) if q.ndim == 3 else (d[0], i[0])
    return _REF[key]


def assert_same(got, want, what):
    np.testing.assert_array_equal(got[1], want[1], err_msg=what + ": indices")
    assert got[0].dtype == np.float32 and got[0].tobytes() == want[0].tobytes(), what + ": distance bits"


@pytest.mark.parametrize("name,k", [(n, k) for n in CASES for k in CASES[n][2]])
def test_mode0_is_the_brute_force_bit_for_bit(kq, name, k):
    q, t, _ = CASES[name]
    got = hip_knn(kq, q, t, k, 0)
    assert got[0].shape == q.shape[:-1] + (k,) and got[1].dtype == np.int32
    assert_same(got, reference(name, k, 0), "%s k=%d" % (name, k))
    if name == "nonfinite_targets":
        assert not np.isin(got[1], [17, 203]).any()
        clean = np.delete(t, [17, 203], axis=0)                     # everything else: as if the two were not there
        d2, i2 = hip_knn(kq, q[:64], clean, k, 0)
        remap = np.delete(np.arange(300), [17, 203])
        np.testing.assert_array_equal(remap[i2], got[1][:64])
        assert d2.tobytes() == got[0][:64].tobytes()
        assert (got[1][64:] == -1).all() and np.isinf(got[0][64:]).all()      # non-finite queries list nothing
    if name == "nt3_k5":
        assert (got[1][:, 3:] == -1).all() and np.isposinf(got[0][:, 3:]).all()


# the tiny cases (<= 64 x 64 pairs), fused arithmetic emulated with exact rationals
TINY = {"nt1": [1, 5], "nt3_k5": [5], "identical": [8], "lattice64": [1, 5, 8], "dup64": [2, 5], "offset64": [5]}


def _tiny_inputs(name):
    if name == "lattice64":
        q, t, _ = CASES["lattice"]
        return q[30:94], np.ascontiguousarray(t.reshape(8, 8, 8, 3)[2:6, 2:6, 2:6].reshape(-1, 3))
    if name == "dup64":
        q, t, _ = CASES["dup10"]
        return q[40:90], np.concatenate([t[0:32], t[90:122]])
    if name == "offset64":
        q, t, _ = CASES["offset_1e3"]
        return q[:64], t[:64]
    return CASES[name][0][:64], CASES[name][1][:64]


@pytest.mark.parametrize("name,k", [(n, k) for n in TINY for k in TINY[n]])
def test_mode1_tiny_cases_exact_rationals(kq, name, k):
    q, t = _tiny_inputs(name)
    assert len(q) <= 64 and len(t) <= 64
    key = ("tiny", name)
    if key not in _REF:
        _REF[key] = sqdist_fma_exact(q, t)
    assert_same(hip_knn(kq, q, t, k, 1), select_k(_REF[key], k), "%s k=%d mode 1" % (name, k))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["clustered5000", "batch3", "far_outside", "lattice", "offset_1e3"])
def test_column0_is_nm_distance_and_the_oracle(kq, oracle, name, mode):
    torch = kq["torch"]
    q, t, _ = CASES[name]
    d, i = hip_knn(kq, q, t, 5, mode)
    qb, tb = (q, t) if q.ndim == 3 else (q[None], t[None])
    d, i = d.reshape(qb.shape[0], -1, 5), i.reshape(qb.shape[0], -1, 5)
    prev = kq["lib"].genpc_set_arith(mode)
    try:
        Q, T = torch.from_numpy(np.ascontiguousarray(qb)).cuda(), torch.from_numpy(np.ascontiguousarray(tb)).cuda()
        nd = torch.empty(qb.shape[:2], device="cuda")
        ni = torch.empty(qb.shape[:2], device="cuda", dtype=torch.int32)
        assert kq["ch"].nm_distance(Q, T, nd, ni) == 1
        torch.cuda.synchronize()
    finally:
        kq["lib"].genpc_set_arith(prev)
    assert nd.cpu().numpy().tobytes() == np.ascontiguousarray(d[:, :, 0]).tobytes()
    np.testing.assert_array_equal(ni.cpu().numpy(), i[:, :, 0])
    e1, _, j1, _ = oracle.chamfer_forward(np.ascontiguousarray(qb), np.ascontiguousarray(tb), mode)
    assert e1.tobytes() == np.ascontiguousarray(d[:, :, 0]).tobytes()
    np.testing.assert_array_equal(j1, i[:, :, 0])


@pytest.mark.parametrize("mode", [0, 1])
def test_self_query_k20_reproduces_the_oracles_mean_distance(kq, oracle, mode):
    P = CASES["clustered5000"][1].copy()
    P[100:110] = P[0:10]                                     # several zero distances
    d, i = hip_knn(kq, P, P, 20, mode)
    assert (d[:, 0] == 0).all() and (np.diff(d.view(np.uint32).astype(np.int64), axis=1) >= 0).all()
    mean = (np.add.accumulate(np.sqrt(d.astype(np.float64)), axis=1)[:, -1] / 20.0).astype(np.float32)
    np.testing.assert_array_equal(mean, oracle.knn_mean_distance(P, 20, mode))
    same = d[:, 1:] == d[:, :-1]                             # among bit-equal distances the lower index first
    assert (i[:, 1:][same] > i[:, :-1][same]).all()
    assert (np.sort(i, axis=1)[:, 1:] != np.sort(i, axis=1)[:, :-1]).all()      # no target twice


def test_api(kq):
    torch = kq["torch"]
    q, t, _ = CASES["nq257"]
    Q, T = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
    for k in (0, 33):
        with pytest.raises(ValueError):
            kq["knn"](Q, T, k)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        kq["knn"](torch.from_numpy(q), torch.from_numpy(t), 3)
    with pytest.raises(ValueError):
        kq["knn"](Q, T[:0], 3)
    d0, i0 = kq["knn"](Q[:0], T, 3)                          # no queries: nothing to do
    assert d0.shape == (0, 3) and i0.shape == (0, 3)
    lib = kq["lib"]
    out_d, out_i = torch.full((257, 3), 7.0, device="cuda"), torch.full((257, 3), 7, device="cuda", dtype=torch.int32)
    for k, nt in ((0, 700), (33, 700), (3, 0)):              # refused, and nothing written
        assert lib.genpc_knn_query(1, 257, Q.data_ptr(), nt, T.data_ptr(), k, out_d.data_ptr(), out_i.data_ptr(), None) == -1
    assert lib.genpc_knn_query(1, 0, Q.data_ptr(), 0, T.data_ptr(), 3, out_d.data_ptr(), out_i.data_ptr(), None) == 1
    assert lib.genpc_knn_query(0, 257, Q.data_ptr(), 700, T.data_ptr(), 3, out_d.data_ptr(), out_i.data_ptr(), None) == 1
    torch.cuda.synchronize()
    assert (out_d == 7.0).all() and (out_i == 7).all()
    a = kq["knn"](Q, T, 5)
    b = kq["knn"](Q, T, 5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])      # two runs, the same bits
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = kq["knn"](Q, T, 5)
    s.synchronize()
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    d3, i3 = kq["knn"](Q[None], T[None], 5)                  # the batched form of the same call
    assert d3.shape == (1, 257, 5) and torch.equal(d3[0], a[0]) and torch.equal(i3[0], a[1])
