"""genpc_nm_distance_ragged (csrc/nn_ragged.hip, the ragged build of csrc/grid.hip) and the layers above it on the GPU.

The yardstick is oracle.chamfer_forward per pair on the CPU, in both fma_modes against the library in both arithmetic
modes; in addition every result is compared with genpc_nm_distance on that pair alone.  Everything bit for bit: distances
as uint32 views, indices as int32.

The search has ONE path (a lane walks its pair's grid; a tiny cloud is a one-cell grid).  What varies with the sizes:
  * the build's pieces per cloud: c >= 32 -> 1 (test_pairs_do_not_leak, c = 36), c >= 8 -> 2 (the c = 24 call), else 4 (c = 1 .. 7);
  * a pair's grid budget, ragged_cells_max(M) = min(M + 64, 15360) cells and ragged_cells_target(M) = clamp(M / 2, 8, 3/4 of that):
    M = 1, 2, 7 take the floor of 8 (in fact one cell), M = 64 .. 3000 take M / 2, M = 24000 (test_single_pair) meets both the
    15360 cap and the 11520 clamp;
  * the work split: a workgroup serves 64 queries of one pair, so N = 63, 64, 65, 255, 256, 257, 1025 end on, at and past
    its edge, and N = 0 leaves a pair with one idle workgroup (or none, when it is the last)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64
POISON_F = np.array([0xDEADBEEF], np.uint32).view(np.float32)[0]
POISON_I = np.int32(-559038737)


@pytest.fixture(scope="module")
def rg():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib, chamfer_3D
    return dict(torch=torch, L=_lib, lib=_lib.lib, ch=chamfer_3D)


class arith:
    def __init__(self, rg, mode):
        self.lib, self.mode = rg["lib"], mode

    def __enter__(self):
        self.prev = self.lib.genpc_set_arith(self.mode)

    def __exit__(self, *a):
        self.lib.genpc_set_arith(self.prev)


def offsets(clouds):
    return [0] + list(np.cumsum([len(c) for c in clouds]))


def packed(clouds):
    return np.ascontiguousarray(np.concatenate([c.reshape(-1, 3) for c in clouds] + [np.zeros((0, 3), np.float32)]).astype(np.float32))


def ragged(rg, pairs, mode, stream=None):
    """One library call over `pairs` = [(queries [N,3], targets [M,3])]; the outputs sit between poisoned guards, which must
    survive.  -> per pair (dist [N] float32, idx [N] int32)."""
    torch = rg["torch"]
    noff, moff = offsets([q for q, _ in pairs]), offsets([t for _, t in pairs])
    n = int(noff[-1])
    dbuf = torch.from_numpy(np.full(n + 2 * GUARD, POISON_F, np.float32)).cuda()
    ibuf = torch.from_numpy(np.full(n + 2 * GUARD, POISON_I, np.int32)).cuda()
    Q, T = torch.from_numpy(packed([q for q, _ in pairs])).cuda(), torch.from_numpy(packed([t for _, t in pairs])).cuda()
    torch.cuda.synchronize()
    with arith(rg, mode):
        if stream is None:
            rc = rg["ch"].nm_distance_ragged(Q, noff, T, moff, dbuf[GUARD:GUARD + n], ibuf[GUARD:GUARD + n])
        else:
            with torch.cuda.stream(stream):
                rc = rg["ch"].nm_distance_ragged(Q, noff, T, moff, dbuf[GUARD:GUARD + n], ibuf[GUARD:GUARD + n])
    assert rc == 1, rg["L"].last_error()
    torch.cuda.synchronize()
    d, i = dbuf.cpu().numpy(), ibuf.cpu().numpy()
    for g in (slice(0, GUARD), slice(GUARD + n, None)):
        assert (d[g].view(np.uint32) == 0xDEADBEEF).all() and (i[g] == POISON_I).all(), "a guard element was written"
    d, i = d[GUARD:GUARD + n], i[GUARD:GUARD + n]
    return [(d[a:b], i[a:b]) for a, b in zip(noff[:-1], noff[1:])]


def nm_alone(rg, q, t, mode):
    """genpc_nm_distance(1, N, .., M, ..) for one pair."""
    torch = rg["torch"]
    Q, T = torch.from_numpy(np.ascontiguousarray(q[None])).cuda(), torch.from_numpy(np.ascontiguousarray(t[None])).cuda()
    d = torch.empty((1, len(q)), device="cuda")
    i = torch.empty((1, len(q)), device="cuda", dtype=torch.int32)
    with arith(rg, mode):
        assert rg["ch"].nm_distance(Q, T, d, i) == 1
    torch.cuda.synchronize()
    return d.cpu().numpy()[0], i.cpu().numpy()[0]


_ORACLE = {}


def oracle_pair(oracle, key, q, t, mode):
    """(dist, idx) of q -> t from the oracle; computed once per (key, mode) and shared."""
    if (key, mode) not in _ORACLE:
        d1, _, i1, _ = oracle.chamfer_forward(np.ascontiguousarray(q[None]), np.ascontiguousarray(t[None]), mode)
        _ORACLE[(key, mode)] = (d1[0], i1[0])
    return _ORACLE[(key, mode)]


def same(got, want, what):
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32
    assert np.array_equal(got[0].view(np.uint32), np.ascontiguousarray(want[0], np.float32).view(np.uint32)), what + ": distances differ"
    assert np.array_equal(got[1], np.asarray(want[1], np.int32)), what + ": indices differ"


def check_pairs(rg, oracle, name, pairs, mode, got=None):
    got = ragged(rg, pairs, mode) if got is None else got
    assert len(got) == len(pairs)
    for j, (q, t) in enumerate(pairs):
        assert got[j][0].shape == (len(q),)
        if len(q) == 0:
            continue
        assert (got[j][1] >= 0).all() and (got[j][1] < len(t)).all(), "%s pair %d: an index is not local" % (name, j)
        same(got[j], oracle_pair(oracle, (name, j), q, t, mode), "%s pair %d (N %d, M %d) mode %d vs the oracle" % (name, j, len(q), len(t), mode))
        same(got[j], nm_alone(rg, q, t, mode), "%s pair %d (N %d, M %d) mode %d vs genpc_nm_distance" % (name, j, len(q), len(t), mode))
    return got


def uniform(rng, n):
    return rng.random((n, 3), dtype=np.float32) - np.float32(0.5)


def clustered(rng, n):
    c = rng.random((5, 3)) - 0.5
    return (c[rng.integers(0, 5, n)] + 0.02 * rng.normal(size=(n, 3))).astype(np.float32)


# ---- 1. boundaries of the work split ----
NS24 = [1, 63, 64, 65, 255, 256, 257, 1025, 2049, 128, 129, 0, 1, 63, 64, 65, 255, 256, 257, 1025, 300, 777, 4097, 0]
MS24 = [513, 1, 3000, 7, 64, 2, 3000, 64, 513, 1, 7, 0, 2, 3000, 1, 513, 7, 64, 2, 3000, 513, 64, 3000, 7]


def _split_pairs():
    rng = np.random.default_rng(20261018)
    assert len(NS24) == len(MS24) == 24 and NS24[11] == 0 and NS24[23] == 0
    return [((clustered if j % 3 == 0 else uniform)(rng, n), (clustered if j % 2 == 0 else uniform)(rng, m)) for j, (n, m) in enumerate(zip(NS24, MS24))]


SPLIT = _split_pairs()


@pytest.mark.parametrize("mode", [0, 1])
def test_work_split_boundaries_c24(rg, oracle, mode):
    check_pairs(rg, oracle, "split24", SPLIT, mode)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,m", [(1, 1), (65, 2), (300, 24000)])
def test_single_pair(rg, oracle, n, m, mode):
    rng = np.random.default_rng(1000 * n + m)
    check_pairs(rg, oracle, "single_%d_%d" % (n, m), [(uniform(rng, n), clustered(rng, m))], mode)


# ---- 2. pairs do not leak into each other ----
def _frames():
    rng = np.random.default_rng(77)
    pairs = []
    for j in range(36):
        scale = np.float32([1e-3, 1.0, 1e3][j % 3])
        shift = (np.float32([1e3, -2e3, 5e2]) * np.float32((j % 5) - 2) * scale).astype(np.float32)
        n, m = int(rng.integers(1, 400)), int(rng.integers(1, 600))
        pairs.append(((uniform(rng, n) * scale + shift).astype(np.float32), (uniform(rng, m) * scale + shift).astype(np.float32)))
    return pairs


FRAMES = _frames()


@pytest.mark.parametrize("mode", [0, 1])
def test_pairs_do_not_leak(rg, oracle, mode):
    fwd = check_pairs(rg, oracle, "frames", FRAMES, mode)
    back = ragged(rg, FRAMES[::-1], mode)[::-1]
    for j in range(len(FRAMES)):
        same(back[j], fwd[j], "pair %d after reversing the order of the pairs" % j)


# ---- 3. ties and degenerate grids ----
def _ties():
    rng = np.random.default_rng(5)
    g = np.arange(8, dtype=np.float32) / np.float32(8)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    one = np.tile(np.float32([0.25, -0.5, 3.0]), (300, 1))
    line = np.zeros((200, 3), np.float32)
    line[:, 0] = rng.random(200, dtype=np.float32)
    plane = uniform(rng, 400)
    plane[:, 2] = np.float32(0.125)
    dup = uniform(rng, 500)
    dup[250:300] = dup[0:50]                                  # later copies of the first 50
    dup[400:420] = dup[10:30]
    crop = uniform(rng, 700)
    padded = crop[np.arange(1000) % 700]                      # the Waymo fixture's pad-repeat
    p = {}
    p["lattice_self"] = (lat, lat)
    p["lattice_shifted"] = (lat + np.float32(1 / 16), lat)    # every query midway between 8 lattice points
    p["identical_targets"] = (np.concatenate([uniform(rng, 100), one[:3]]), one)
    p["line"] = (uniform(rng, 150), line)
    p["plane"] = (uniform(rng, 150), plane)
    p["coincident"] = (dup.copy(), dup)
    p["padded_targets"] = (uniform(rng, 300), padded)
    p["padded_queries"] = (padded, crop[::-1].copy())
    return p


TIES = _ties()


@pytest.mark.parametrize("mode", [0, 1])
def test_ties_and_degenerate_grids(rg, oracle, mode):
    names = list(TIES)
    got = check_pairs(rg, oracle, "ties", [TIES[k] for k in names], mode)
    r = dict(zip(names, got))
    d, i = r["lattice_self"]
    assert (d == 0).all() and np.array_equal(i, np.arange(512))
    d, i = r["lattice_shifted"]
    assert (d == np.float32(3 / 256)).all()                   # eight targets at the same bits: the lowest index
    d, i = r["identical_targets"]
    assert (i == 0).all() and (d[-3:] == 0).all()
    d, i = r["coincident"]
    assert (d == 0).all()
    want = np.arange(500)
    want[250:300] = np.arange(0, 50)
    want[400:420] = np.arange(10, 30)
    assert np.array_equal(i, want)                            # the first of the duplicates
    d, i = r["padded_targets"]
    assert (i < 700).all()                                    # never a repeated copy


# ---- 4. rectangular agreement ----
@pytest.mark.parametrize("mode", [0, 1])
def test_rectangular_agreement(rg, golden, mode):
    torch = rg["torch"]
    z = golden("chamfer_seed0_b2_1000x777.npz")
    rng = np.random.default_rng(3)
    x1 = np.concatenate([z["xyz1"], uniform(rng, 1000)[None]])
    x2 = np.concatenate([z["xyz2"], uniform(rng, 777)[None]])
    for a, b, dk, ik in ((x1, x2, "dist1_m%d", "idx1_m%d"), (x2, x1, "dist2_m%d", "idx2_m%d")):
        got = ragged(rg, [(a[j], b[j]) for j in range(3)], mode)
        A, B = torch.from_numpy(np.ascontiguousarray(a)).cuda(), torch.from_numpy(np.ascontiguousarray(b)).cuda()
        d = torch.empty(a.shape[:2], device="cuda")
        i = torch.empty(a.shape[:2], device="cuda", dtype=torch.int32)
        with arith(rg, mode):
            assert rg["ch"].nm_distance(A, B, d, i) == 1
        torch.cuda.synchronize()
        d, i = d.cpu().numpy(), i.cpu().numpy()
        for j in range(3):
            same(got[j], (d[j], i[j]), "pair %d vs the batched call" % j)
        for j in range(2):
            same(got[j], (z[dk % mode][j], z[ik % mode][j]), "pair %d vs the recorded values" % j)


# ---- 5. real data ----
def _waymo(golden, count):
    z = golden("waymo_car59_4096.npz")
    sizes = np.minimum(z["counts"][:count], 4096)
    return [np.ascontiguousarray(z["crops"][j, :sizes[j]]) for j in range(count)], np.ascontiguousarray(z["complete"])


@pytest.mark.parametrize("mode", [0, 1])
def test_waymo_crops_at_their_true_counts(rg, oracle, golden, mode):
    torch = rg["torch"]
    from genpc_amd.loss_functions.Chamfer3D.dist_chamfer_ragged import chamfer_ragged
    crops, complete = _waymo(golden, 8)
    assert len({len(c) for c in crops}) > 1
    with arith(rg, mode):
        d1, d2, i1, i2, o1, o2 = chamfer_ragged([torch.from_numpy(c).cuda() for c in crops], [torch.from_numpy(complete).cuda()] * 8)
    torch.cuda.synchronize()
    assert o1.tolist() == offsets(crops) and o2.tolist() == [4096 * j for j in range(9)]
    d1, d2, i1, i2 = (t.cpu().numpy() for t in (d1, d2, i1, i2))
    for j, c in enumerate(crops):
        key = ("waymo8", j, mode)
        if key not in _ORACLE:
            _ORACLE[key] = oracle.chamfer_forward(c[None], complete[None], mode)
        e1, e2, j1, j2 = _ORACLE[key]
        same((d1[o1[j]:o1[j + 1]], i1[o1[j]:o1[j + 1]]), (e1[0], j1[0]), "crop %d -> complete" % j)
        same((d2[o2[j]:o2[j + 1]], i2[o2[j]:o2[j + 1]]), (e2[0], j2[0]), "complete -> crop %d" % j)


def test_evaluate_clouds_against_float64_means_of_the_oracle(rg, oracle, golden):
    torch = rg["torch"]
    from genpc_amd.metric import evaluate_clouds
    crops, complete = _waymo(golden, 8)
    mode = rg["lib"].genpc_get_arith()
    table = evaluate_clouds([torch.from_numpy(c).cuda() for c in crops], [torch.from_numpy(complete).cuda()] * 8)
    assert table.dtype == torch.float64 and tuple(table.shape) == (8, 2) and table.is_cuda
    table = table.cpu().numpy()
    want = np.zeros((8, 2))
    for j, c in enumerate(crops):
        key = ("waymo8", j, mode)
        if key not in _ORACLE:
            _ORACLE[key] = oracle.chamfer_forward(c[None], complete[None], mode)
        e1, e2, _, _ = _ORACLE[key]
        want[j, 0] = (np.sqrt(e1[0]).astype(np.float64).mean() + np.sqrt(e2[0]).astype(np.float64).mean()) / 2      # fp32 sqrt, float64 mean
        want[j, 1] = e1[0].astype(np.float64).mean() + e2[0].astype(np.float64).mean()
    print("evaluate_clouds relative error:", np.abs(table / want - 1).max())
    np.testing.assert_allclose(table, want, rtol=1e-9, atol=0)


def test_evaluate_clouds_agrees_with_evaluate_scans_on_rectangular_input(rg, golden):
    """fp32 cascade sums of evaluate_scans against float64 segment sums: (log2 N + a few) 2^-24 at N = 4096 is about 1e-6; the
    issue's bound, with its tenfold margin, is 1e-5."""
    torch = rg["torch"]
    from genpc_amd.metric import evaluate_clouds, evaluate_scans
    z = golden("waymo_car59_4096.npz")
    pred = torch.from_numpy(np.ascontiguousarray(z["crops"][:2])).cuda()
    gt = torch.from_numpy(np.ascontiguousarray(z["complete"])).cuda().unsqueeze(0).repeat(2, 1, 1).contiguous()
    rect = evaluate_scans(pred, gt)[:, :2].double().cpu().numpy()
    rag = evaluate_clouds((pred.reshape(-1, 3), [0, 4096, 8192]), list(gt)).cpu().numpy()
    print("evaluate_clouds vs evaluate_scans relative difference:", np.abs(rag / rect - 1).max())
    np.testing.assert_allclose(rag, rect, rtol=1e-5, atol=0)


# ---- 6. the non-finite contract ----
@pytest.mark.parametrize("mode", [0, 1])
def test_non_finite_contract(rg, oracle, mode):
    rng = np.random.default_rng(6)
    qa, ta = uniform(rng, 130), uniform(rng, 200)
    qa[7, 1] = np.nan
    qa[129, 0] = -np.inf
    qb, tb = uniform(rng, 70), uniform(rng, 900)
    tb[450, 2] = np.inf
    qc, tc = uniform(rng, 300), uniform(rng, 333)
    got = ragged(rg, [(qa, ta), (qb, tb), (qc, tc)], mode)
    d, i = got[0]
    bad = np.zeros(130, bool)
    bad[[7, 129]] = True
    assert np.isnan(d[bad]).all() and (i[bad] == -1).all()
    fin = ~bad                                               # the pair's finite queries are answered as ever
    same((d[fin], i[fin]), oracle_pair(oracle, ("nonfinite", "a"), qa[fin], ta, mode), "finite queries beside a NaN query")
    d, i = got[1]
    assert np.isnan(d).all() and (i == -1).all()
    same(got[2], oracle_pair(oracle, ("nonfinite", "c"), qc, tc, mode), "the finite pair")


# ---- 7. arguments ----
def test_bad_arguments_are_refused_and_write_nothing(rg):
    torch, lib = rg["torch"], rg["lib"]
    rng = np.random.default_rng(8)
    Q, T = torch.from_numpy(uniform(rng, 20)).cuda(), torch.from_numpy(uniform(rng, 30)).cuda()
    d = torch.from_numpy(np.full(20, POISON_F, np.float32)).cuda()
    i = torch.from_numpy(np.full(20, POISON_I, np.int32)).cuda()

    def call(c, noff, moff):
        na, ma = (ctypes.c_int * len(noff))(*noff), (ctypes.c_int * len(moff))(*moff)
        vp = lambda a: ctypes.cast(a, ctypes.c_void_p)      # noqa: E731
        return lib.genpc_nm_distance_ragged(c, vp(na), rg["L"].ptr(Q), vp(ma), rg["L"].ptr(T), rg["L"].ptr(d), rg["L"].ptr(i),
                                            rg["L"].stream_of(Q))
    for what, c, noff, moff in (("a pair with queries and no targets", 2, [0, 10, 20], [0, 30, 30]),
                                ("decreasing query offsets", 2, [0, 15, 10], [0, 10, 30]),
                                ("decreasing target offsets", 2, [0, 10, 20], [0, 20, 10]),
                                ("noff[0] != 0", 2, [5, 10, 20], [0, 10, 30]),
                                ("negative c", -1, [0, 10, 20], [0, 10, 30]),
                                ("too many pairs", 385, [0] * 386, [0] * 386)):
        rc = call(c, noff, moff)
        assert rc == -1, what
        assert "genpc_nm_distance_ragged" in rg["L"].last_error(), what
    assert call(0, [0], [0]) == 1
    assert call(2, [0, 0, 0], [0, 10, 30]) == 1             # no queries in total
    torch.cuda.synchronize()
    assert (d.cpu().numpy().view(np.uint32) == 0xDEADBEEF).all() and (i.cpu().numpy() == POISON_I).all()


# ---- 8. determinism and streams ----
def test_same_bytes_twice_and_on_another_stream(rg):
    torch = rg["torch"]
    pairs = SPLIT[:12]
    a = ragged(rg, pairs, 1)
    b = ragged(rg, pairs, 1)
    s = torch.cuda.Stream()
    c = ragged(rg, pairs, 1, stream=s)
    for j in range(len(pairs)):
        same(b[j], a[j], "second call, pair %d" % j)
        same(c[j], a[j], "side stream, pair %d" % j)
