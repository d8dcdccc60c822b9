"""The all-pairs ragged nearest neighbours (csrc/nn_ragged_dense.hip, opt-in through genpc_nn_ragged_tune / search="dense") on the GPU.

Three yardsticks per pair, everything bit for bit (distances as uint32 views, indices as int32), in both arithmetic modes:
oracle.chamfer_forward on the CPU, genpc_nm_distance on the pair alone, and the grid call (search="grid") on the same batch.
The outputs sit between poisoned guards, which must survive.  Helpers and case lists are tests/test_gpu_nn_ragged.py's.

What varies with the sizes, all of it read from the exported plan (genpc_nn_ragged_dense_plan), none typed in:
  * targets pass through LDS in tiles of `tile`, of which wave w scans [w share, (w + 1) share): M = 1, 2, share - 1 / share /
    share + 1, tile - 1 / tile / tile + 1, 2 tile + 1, and 24000 (24 tiles, the last one partial);
  * an item is 64 queries of a pair: N = 1, 63, 64, 65, 257 and 0 (an idle workgroup, or none when the pair is the last)."""
import ctypes
import threading

import numpy as np
import pytest

from test_gpu_nn_ragged import (FRAMES, GUARD, POISON_F, POISON_I, SPLIT, TIES, arith, check_pairs, clustered, nm_alone, offsets,
                                oracle_pair, packed, ragged, rg, same, uniform)      # noqa: F401  (rg: the fixture)

pytestmark = pytest.mark.gpu


def dense(rg, pairs, mode, stream=None, search="dense"):
    """test_gpu_nn_ragged.ragged with the keyword: one call over `pairs`, the outputs between poisoned guards."""
    torch = rg["torch"]
    noff, moff = offsets([q for q, _ in pairs]), offsets([t for _, t in pairs])
    n = int(noff[-1])
    dbuf = torch.from_numpy(np.full(n + 2 * GUARD, POISON_F, np.float32)).cuda()
    ibuf = torch.from_numpy(np.full(n + 2 * GUARD, POISON_I, np.int32)).cuda()
    Q, T = torch.from_numpy(packed([q for q, _ in pairs])).cuda(), torch.from_numpy(packed([t for _, t in pairs])).cuda()
    torch.cuda.synchronize()
    before = rg["lib"].genpc_nn_ragged_tune(0)
    rg["lib"].genpc_nn_ragged_tune(before)
    with arith(rg, mode):
        if stream is None:
            rc = rg["ch"].nm_distance_ragged(Q, noff, T, moff, dbuf[GUARD:GUARD + n], ibuf[GUARD:GUARD + n], search=search)
        else:
            with torch.cuda.stream(stream):
                rc = rg["ch"].nm_distance_ragged(Q, noff, T, moff, dbuf[GUARD:GUARD + n], ibuf[GUARD:GUARD + n], search=search)
    assert rc == 1, rg["L"].last_error()
    after = rg["lib"].genpc_nn_ragged_tune(before)
    assert after == before, "the call left the thread's mode at %d, it was %d" % (after, before)
    torch.cuda.synchronize()
    d, i = dbuf.cpu().numpy(), ibuf.cpu().numpy()
    for g in (slice(0, GUARD), slice(GUARD + n, None)):
        assert (d[g].view(np.uint32) == 0xDEADBEEF).all() and (i[g] == POISON_I).all(), "a guard element was written"
    d, i = d[GUARD:GUARD + n], i[GUARD:GUARD + n]
    return [(d[a:b], i[a:b]) for a, b in zip(noff[:-1], noff[1:])]


def three_yardsticks(rg, oracle, name, pairs, mode):
    """dense == the oracle == genpc_nm_distance on the pair alone (check_pairs), and == the grid call on the same batch."""
    got = check_pairs(rg, oracle, name, pairs, mode, got=dense(rg, pairs, mode))
    grid = dense(rg, pairs, mode, search="grid")
    for j in range(len(pairs)):
        same(got[j], grid[j], "%s pair %d (N %d, M %d) mode %d vs the grid call" % (name, j, len(pairs[j][0]), len(pairs[j][1]), mode))
    return got


@pytest.fixture(scope="module")
def plan(rg):
    """The exported constants: (tile, share)."""
    z = (ctypes.c_int * 1)(0)
    out = (ctypes.c_int * 8)()
    assert rg["lib"].genpc_nn_ragged_dense_plan(0, ctypes.cast(z, ctypes.c_void_p), ctypes.cast(z, ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p)) == 1
    assert out[1] == 256 and out[2] == 64 and out[3] == 4 * out[4] and out[3] >= 64
    return out[3], out[4]


# ---- 1. the grid tests' batches ----
@pytest.mark.parametrize("mode", [0, 1])
def test_work_split_boundaries_c24(rg, oracle, mode):
    three_yardsticks(rg, oracle, "split24", SPLIT, mode)          # (the names of test_gpu_nn_ragged: the oracle's answers are shared)


@pytest.mark.parametrize("mode", [0, 1])
def test_frames_c36_and_reversed(rg, oracle, mode):
    fwd = three_yardsticks(rg, oracle, "frames", FRAMES, mode)
    back = dense(rg, FRAMES[::-1], mode)[::-1]
    for j in range(len(FRAMES)):
        same(back[j], fwd[j], "pair %d after reversing the order of the pairs" % j)


# ---- 2. edges of the tile, of a wave's share and of the item ----
_EDGES = {}


def _edges(plan):
    if not _EDGES:
        tile, share = plan
        ms = [1, 2, share - 1, share, share + 1, tile - 1, tile, tile + 1, 2 * tile + 1]
        ns = [1, 63, 64, 65, 257]
        rng = np.random.default_rng(20261020)
        pairs = []
        for j in range(36):
            if j in (17, 35):                                  # the empty pair in the middle and at the end
                pairs.append((uniform(rng, 0), uniform(rng, 5)))
                continue
            n, m = ns[j % 5], ms[(j * 2 + j // 9) % 9]
            pairs.append(((clustered if j % 3 == 0 else uniform)(rng, n), (clustered if j % 2 == 0 else uniform)(rng, m)))
        assert {len(t) for _, t in pairs} >= set(ms) and {len(q) for q, _ in pairs} >= set(ns + [0])
        _EDGES["c36"] = pairs
        _EDGES["big"] = [(uniform(rng, 257), clustered(rng, 24000))]
        _EDGES["c1"] = [[(uniform(rng, n), uniform(rng, m))] for n, m in ((1, 1), (65, share + 1), (64, tile), (257, 2 * tile + 1), (63, tile + 1))]
    return _EDGES


@pytest.mark.parametrize("mode", [0, 1])
def test_edges_c36_and_reversed(rg, oracle, plan, mode):
    pairs = _edges(plan)["c36"]
    fwd = three_yardsticks(rg, oracle, "dense_edges36", pairs, mode)
    back = dense(rg, pairs[::-1], mode)[::-1]
    for j in range(len(pairs)):
        same(back[j], fwd[j], "pair %d after reversing the order of the pairs" % j)


@pytest.mark.parametrize("mode", [0, 1])
def test_edges_c1(rg, oracle, plan, mode):
    e = _edges(plan)
    three_yardsticks(rg, oracle, "dense_big", e["big"], mode)
    for k, pairs in enumerate(e["c1"]):
        three_yardsticks(rg, oracle, "dense_c1_%d" % k, pairs, mode)


# ---- 3. misaligned pairs: no query has a near target ----
def _misaligned(plan):
    tile, share = plan
    rng = np.random.default_rng(31)
    pairs = []
    for n, m, axis in ((300, tile + 300, 0), (900, 4500, 1), (65, share + 1, 2), (257, 700, 1)):
        t = clustered(rng, m)
        c = t.astype(np.float64).mean(0)
        diam = float(np.linalg.norm(t.max(0) - t.min(0)))
        flip = -np.ones(3)
        flip[axis] = 1.0                                        # a turn by 180 degrees about `axis` through the centre
        push = np.zeros(3)
        push[(axis + 1) % 3] = 4.0 * diam
        q = (c + (t[rng.permutation(m)[:n]].astype(np.float64) - c) * flip + push).astype(np.float32)
        assert np.linalg.norm(q[:, None, :].astype(np.float64) - t[None, ::7], axis=-1).min() > 2.0 * diam
        pairs.append((q, t))
    return pairs


@pytest.mark.parametrize("mode", [0, 1])
def test_misaligned_pairs(rg, oracle, plan, mode):
    three_yardsticks(rg, oracle, "dense_misaligned", _misaligned(plan), mode)


# ---- 4. ties ----
@pytest.mark.parametrize("mode", [0, 1])
def test_ties(rg, oracle, plan, mode):
    tile, share = plan
    names = list(TIES)
    got = three_yardsticks(rg, oracle, "ties", [TIES[k] for k in names], mode)
    r = dict(zip(names, got))
    assert np.array_equal(r["lattice_self"][1], np.arange(512)) and (r["identical_targets"][1] == 0).all()
    # a tile-sized run of identical targets from the middle of wave 0's share: it crosses every share boundary and the tile's end
    rng = np.random.default_rng(44)
    t = uniform(rng, 2 * tile + 40)
    first = share - 100
    point = np.float32([2.0, -3.0, 0.5])                         # (outside the unit box: nothing else is as near)
    t[first:first + tile] = point
    q = np.concatenate([point[None], point[None] + np.float32(0.01), uniform(rng, 70) + point])
    got = three_yardsticks(rg, oracle, "dense_run", [(q, t), (q[:3], t[first + 1:])], mode)
    assert (got[0][1] == first).all() and (got[1][1] == 0).all()          # the lowest index wins across waves and tiles
    assert got[0][0][0] == 0.0


# ---- 5. distances that overflow ----
@pytest.mark.parametrize("mode", [0, 1])
def test_overflow(rg, oracle, plan, mode):
    tile, share = plan
    rng = np.random.default_rng(55)
    far_q = np.full((70, 3), 3e19, np.float32)
    far_t = np.full((share + 5, 3), -3e19, np.float32)
    some_q = np.full((65, 3), 1e19, np.float32)                 # 3e38 from the unit box: finite; 4.8e39 from -3e19: +inf
    some_t = np.concatenate([np.full((share + 5, 3), -3e19, np.float32), uniform(rng, tile), np.full((9, 3), -3e19, np.float32)])
    got = three_yardsticks(rg, oracle, "dense_overflow", [(far_q, far_t), (some_q, some_t), (far_q[:1], far_t[:1])], mode)
    for k in (0, 2):
        assert np.isposinf(got[k][0]).all() and (got[k][1] == 0).all()          # every distance +inf: (+inf, 0)
    assert np.isfinite(got[1][0]).all() and (got[1][1] >= share + 5).all() and (got[1][1] < share + 5 + tile).all()


# ---- 6. the non-finite contract ----
@pytest.mark.parametrize("mode", [0, 1])
def test_non_finite_contract(rg, oracle, plan, mode):
    tile, share = plan
    rng = np.random.default_rng(6)
    qa, ta = uniform(rng, 130), uniform(rng, 200)
    qa[7, 1] = np.nan
    qa[129, 0] = -np.inf
    qb, tb = uniform(rng, 70), uniform(rng, tile + 100)
    tb[tile + 50, 2] = np.inf                                   # in the last, partial tile
    qc, tc = uniform(rng, 300), uniform(rng, 333)
    pairs = [(qa, ta), (qb, tb), (qc, tc)]
    got = dense(rg, pairs, mode)
    grid = ragged(rg, pairs, mode)
    for j in range(3):
        same(got[j], grid[j], "pair %d vs the grid call" % j)
    d, i = got[0]
    bad = np.zeros(130, bool)
    bad[[7, 129]] = True
    assert np.isnan(d[bad]).all() and (i[bad] == -1).all()
    same((d[~bad], i[~bad]), oracle_pair(oracle, ("dense_nonfinite", "a"), qa[~bad], ta, mode), "finite queries beside a NaN query")
    assert np.isnan(got[1][0]).all() and (got[1][1] == -1).all()
    same(got[2], oracle_pair(oracle, ("dense_nonfinite", "c"), qc, tc, mode), "the finite pair")


# ---- 7. determinism and streams ----
def test_same_bytes_twice_and_on_another_stream(rg):
    torch = rg["torch"]
    pairs = SPLIT[:12]
    a = dense(rg, pairs, 1)
    b = dense(rg, pairs, 1)
    c = dense(rg, pairs, 1, stream=torch.cuda.Stream())
    for j in range(len(pairs)):
        same(b[j], a[j], "second call, pair %d" % j)
        same(c[j], a[j], "side stream, pair %d" % j)


# ---- 8. the mode ----
def test_mode_handling(rg):
    lib, L = rg["lib"], rg["L"]
    assert lib.genpc_nn_ragged_tune(0) == 0
    assert lib.genpc_nn_ragged_tune(2) == -1 and "genpc_nn_ragged_tune" in L.last_error()
    assert lib.genpc_nn_ragged_tune(0) == 0                     # the refused value left the mode
    dense(rg, SPLIT[:3], 1)                                     # (asserts that the call restores the mode)
    assert lib.genpc_nn_ragged_tune(1) == 0
    try:
        seen = []
        th = threading.Thread(target=lambda: seen.append(lib.genpc_nn_ragged_tune(0)))
        th.start()
        th.join()
        assert seen == [0]                                      # a second host thread starts in grid mode
        a = dense(rg, SPLIT[:3], 1, search=None)                # the thread's mode: dense
        b = dense(rg, SPLIT[:3], 1, search="grid")
        assert lib.genpc_nn_ragged_tune(1) == 1                 # ... and still dense behind a "grid" call
        for j in range(3):
            same(a[j], b[j], "pair %d, the thread's mode against the keyword" % j)
    finally:
        lib.genpc_nn_ragged_tune(0)
    with pytest.raises(ValueError, match='"grid" or "dense"'):
        dense(rg, SPLIT[:1], 1, search="brute")


# ---- 9. refusals ----
def test_refusals_write_nothing(rg):
    torch, lib, L = rg["torch"], rg["lib"], rg["L"]
    rng = np.random.default_rng(9)
    Q, T = torch.from_numpy(uniform(rng, 20)).cuda(), torch.from_numpy(uniform(rng, 30)).cuda()      # far shorter than the tables claim
    d = torch.from_numpy(np.full(20, POISON_F, np.float32)).cuda()
    i = torch.from_numpy(np.full(20, POISON_I, np.int32)).cuda()
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)              # noqa: E731

    def tables(n, m):
        return (ctypes.c_int * 2)(0, n), (ctypes.c_int * 2)(0, m)
    h = (1 << 18) + 1
    out = (ctypes.c_int * 8)()
    assert lib.genpc_nn_ragged_tune(1) == 0
    try:
        for n, m, word in ((h, h, "2^36"), (2, (1 << 20) + 1, "2^20")):
            na, ma = tables(n, m)
            assert lib.genpc_nn_ragged_dense_plan(1, vp(na), vp(ma), vp(out)) == -1
            assert "genpc_nn_ragged_dense_plan" in L.last_error() and word in L.last_error()
            rc = lib.genpc_nm_distance_ragged(1, vp(na), L.ptr(Q), vp(ma), L.ptr(T), L.ptr(d), L.ptr(i), L.stream_of(Q))
            assert rc == -1 and "genpc_nm_distance_ragged" in L.last_error() and word in L.last_error()
        na, ma = tables(20, 30)                                 # the same buffers with a table that fits them: served
        assert lib.genpc_nn_ragged_dense_plan(1, vp(na), vp(ma), vp(out)) == 1 and out[0] == 1
    finally:
        lib.genpc_nn_ragged_tune(0)
    torch.cuda.synchronize()
    assert (d.cpu().numpy().view(np.uint32) == 0xDEADBEEF).all() and (i.cpu().numpy() == POISON_I).all()
