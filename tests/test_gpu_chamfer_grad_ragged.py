"""genpc_chamfer_backward_ragged (csrc/chamfer_grad_ragged.hip) on the GPU, through chamfer_3D.backward_ragged.

The yardstick is oracle.chamfer_backward per pair on the CPU -- its accumulation order (direction 1 ascending, then
direction 2 ascending) IS the kernel's contract, so every comparison is bit for bit, gradients as uint32 views.  Where an
index is out of range (the oracle would dereference it) the yardstick is tests/chamfer_grad_ragged_ref.py, the
definition as a numpy double loop.  Indices come from the ragged forward; the weights are random with mixed signs and some
exact zeros; the outputs are pre-filled with 0xDEADBEEF and sit between poisoned guards.

The kernels have one path.  What varies with the sizes: a workgroup serves 64 rows of one pair and one side, so N, M = 63, 64,
65, 255, 256, 257, 1025 end on, at and past its edge and an empty pair leaves an idle workgroup per side; the sort's bits follow
the total row count; a row's chain is as long as the number of indices that name it (4097 on the one row of M = 1)."""
import ctypes

import numpy as np
import pytest

import chamfer_grad_ragged_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
POISON_F = np.array([0xDEADBEEF], np.uint32).view(np.float32)[0]


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
    return [0] + [int(v) for v in np.cumsum([len(c) for c in clouds])]


def packed(arrs, tail=()):
    return np.ascontiguousarray(np.concatenate([np.asarray(a) for a in arrs] + [np.zeros((0,) + tuple(tail), arrs[0].dtype)]))


def uniform(rng, n):
    return rng.random((n, 3), dtype=np.float32) - np.float32(0.5)


def clustered(rng, n):
    c = rng.random((5, 3)) - 0.5
    return (c[rng.integers(0, 5, n)] + 0.02 * rng.normal(size=(n, 3))).astype(np.float32)


def weights(rng, n):
    g = rng.normal(size=n).astype(np.float32)
    g[rng.random(n) < 0.1] = 0
    return g


def forward_indices(rg, pairs):
    """(idx1 per pair, idx2 per pair) from the ragged forward, both directions."""
    torch, ch = rg["torch"], rg["ch"]
    noff, moff = offsets([a for a, _ in pairs]), offsets([b for _, b in pairs])
    A = torch.from_numpy(packed([a for a, _ in pairs], (3,))).cuda()
    B = torch.from_numpy(packed([b for _, b in pairs], (3,))).cuda()
    out = []
    for q, qo, t, to in ((A, noff, B, moff), (B, moff, A, noff)):
        d = torch.empty(qo[-1], device="cuda")
        i = torch.empty(qo[-1], device="cuda", dtype=torch.int32)
        assert ch.nm_distance_ragged(q, qo, t, to, d, i) == 1, rg["L"].last_error()
        i = i.cpu().numpy()
        out.append([i[a:b].copy() for a, b in zip(qo[:-1], qo[1:])])
    return out[0], out[1]


def backward(rg, pairs, g1, g2, i1, i2, stream=None):
    """One library call over `pairs` = [(A [N,3], B [M,3])] with per-pair weights and indices; the poisoned outputs sit between
    poisoned guards, which must survive.  -> per pair (gradxyz1 [N,3], gradxyz2 [M,3])."""
    torch, ch = rg["torch"], rg["ch"]
    noff, moff = offsets([a for a, _ in pairs]), offsets([b for _, b in pairs])
    n, m = noff[-1], moff[-1]
    A = torch.from_numpy(packed([a for a, _ in pairs], (3,))).cuda()
    B = torch.from_numpy(packed([b for _, b in pairs], (3,))).cuda()
    G1, G2 = torch.from_numpy(packed(g1)).cuda(), torch.from_numpy(packed(g2)).cuda()
    I1, I2 = torch.from_numpy(packed(i1).astype(np.int32)).cuda(), torch.from_numpy(packed(i2).astype(np.int32)).cuda()
    b1 = torch.from_numpy(np.full(3 * n + 2 * GUARD, POISON_F, np.float32)).cuda()
    b2 = torch.from_numpy(np.full(3 * m + 2 * GUARD, POISON_F, np.float32)).cuda()
    o1, o2 = b1[GUARD:GUARD + 3 * n].view(n, 3), b2[GUARD:GUARD + 3 * m].view(m, 3)
    torch.cuda.synchronize()
    if stream is None:
        rc = ch.backward_ragged(A, noff, B, moff, o1, o2, G1, G2, I1, I2)
    else:
        with torch.cuda.stream(stream):
            rc = ch.backward_ragged(A, noff, B, moff, o1, o2, G1, G2, I1, I2)
    assert rc == 1, rg["L"].last_error()
    torch.cuda.synchronize()
    res = []
    for buf, rows in ((b1, n), (b2, m)):
        h = buf.cpu().numpy()
        for g in (slice(0, GUARD), slice(GUARD + 3 * rows, None)):
            assert (h[g].view(np.uint32) == 0xDEADBEEF).all(), "a guard element was written"
        res.append(h[GUARD:GUARD + 3 * rows].reshape(rows, 3))
    # every row is overwritten.  (A sum can only be the poison's own bits by an accident of 2^-32; none of the cases has one.)
    assert not (res[0].view(np.uint32) == 0xDEADBEEF).any() and not (res[1].view(np.uint32) == 0xDEADBEEF).any(), "a row was left unwritten"
    return [(res[0][a:b], res[1][c:d]) for a, b, c, d in zip(noff[:-1], noff[1:], moff[:-1], moff[1:])]


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same(got, want, what):
    for side in (0, 1):
        g, w = got[side], np.asarray(want[side], np.float32).reshape(-1, 3)
        assert g.shape == w.shape, what
        bad = np.flatnonzero((bits(g) != bits(w)).any(axis=1))
        assert bad.size == 0, "%s: gradxyz%d differs in %d rows, first %d: %s vs %s" % (what, side + 1, bad.size, bad[0], g[bad[0]], w[bad[0]])


def oracle_pair(oracle, a, b, g1, g2, i1, i2):
    if len(a) == 0 and len(b) == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)
    x1, x2 = oracle.chamfer_backward(np.ascontiguousarray(a[None]), np.ascontiguousarray(b[None]), np.ascontiguousarray(g1[None]),
                                     np.ascontiguousarray(g2[None]), np.ascontiguousarray(i1[None]), np.ascontiguousarray(i2[None]))
    return x1[0], x2[0]


class Case:
    """Pairs with their weights, the forward's indices and the oracle's gradients, made once and shared."""
    _made = {}

    def __init__(self, rg, oracle, pairs, seed):
        rng = np.random.default_rng(seed)
        self.pairs = pairs
        self.g1, self.g2 = [weights(rng, len(a)) for a, _ in pairs], [weights(rng, len(b)) for _, b in pairs]
        self.i1, self.i2 = forward_indices(rg, pairs)
        for j, (a, b) in enumerate(pairs):
            assert ((self.i1[j] >= 0) & (self.i1[j] < len(b))).all() and ((self.i2[j] >= 0) & (self.i2[j] < len(a))).all()
        self.want = [oracle_pair(oracle, a, b, self.g1[j], self.g2[j], self.i1[j], self.i2[j]) for j, (a, b) in enumerate(pairs)]

    @classmethod
    def get(cls, name, rg, oracle, make, seed):
        if name not in cls._made:
            cls._made[name] = cls(rg, oracle, make(), seed)
        return cls._made[name]

    def run(self, rg, order=None, stream=None):
        order = list(range(len(self.pairs))) if order is None else order
        pick = lambda xs: [xs[j] for j in order]      # noqa: E731
        got = backward(rg, pick(self.pairs), pick(self.g1), pick(self.g2), pick(self.i1), pick(self.i2), stream)
        out = [None] * len(self.pairs)
        for pos, j in enumerate(order):
            out[j] = got[pos]
        return out

    def check(self, got, what):
        for j, (a, b) in enumerate(self.pairs):
            same(got[j], self.want[j], "%s pair %d (N %d, M %d) vs the oracle" % (what, j, len(a), len(b)))


# ---- 1. the bits of the oracle, per pair ----
NS24 = [1, 63, 64, 65, 255, 256, 257, 1025, 4097, 1, 300, 0, 63, 64, 65, 255, 256, 257, 1025, 129, 777, 2, 513, 0]
MS24 = [513, 1, 3000, 7, 64, 2, 3000, 64, 1, 3000, 513, 0, 2, 3000, 1, 513, 7, 64, 2, 3000, 64, 7, 513, 0]


def _split_pairs():
    rng = np.random.default_rng(20261019)
    assert len(NS24) == len(MS24) == 24 and (NS24[11], MS24[11]) == (0, 0) and (NS24[23], MS24[23]) == (0, 0)
    assert (NS24[8], MS24[8]) == (4097, 1) and (NS24[9], MS24[9]) == (1, 3000)
    assert set(NS24) >= {1, 63, 64, 65, 255, 256, 257, 1025, 4097, 0} and set(MS24) >= {1, 2, 7, 64, 513, 3000, 0}
    return [((clustered if j % 3 == 0 else uniform)(rng, n), (clustered if j % 2 == 0 else uniform)(rng, m)) for j, (n, m) in enumerate(zip(NS24, MS24))]


def _frames():
    rng = np.random.default_rng(78)
    pairs = []
    for j in range(36):
        scale = np.float32([1e-3, 1.0, 1e3][j % 3])
        shift = (np.float32([1e3, -2e3, 5e2]) * np.float32((j % 5) - 2) * scale).astype(np.float32)
        n, m = int(rng.integers(1, 400)), int(rng.integers(1, 600))
        pairs.append(((uniform(rng, n) * scale + shift).astype(np.float32), (uniform(rng, m) * scale + shift).astype(np.float32)))
    return pairs


def _single():
    rng = np.random.default_rng(4)
    return [(clustered(rng, 777), uniform(rng, 300))]


def test_bits_of_the_oracle_c24(rg, oracle):
    case = Case.get("split24", rg, oracle, _split_pairs, 1)
    got = case.run(rg)
    case.check(got, "split24")
    assert np.bincount(case.i1[8], minlength=1)[0] == 4097            # 4097 ordered terms on the one row of pair 8


def test_bits_of_the_oracle_c1(rg, oracle):
    case = Case.get("single", rg, oracle, _single, 2)
    case.check(case.run(rg), "single")


def test_bits_of_the_oracle_c36_frames(rg, oracle):
    case = Case.get("frames", rg, oracle, _frames, 3)
    case.check(case.run(rg), "frames")


# ---- 2. zeros and ties ----
def _ties():
    rng = np.random.default_rng(5)
    g = np.arange(8, dtype=np.float32) / np.float32(8)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    one = np.tile(np.float32([0.25, -0.5, 3.0]), (300, 1))
    dup = uniform(rng, 500)
    dup[250:300] = dup[0:50]                                  # later copies of the first 50
    dup[400:420] = dup[10:30]
    crop = uniform(rng, 700)
    padded = crop[np.arange(1000) % 700]                      # the Waymo fixture's pad-repeat
    p = {}
    p["lattice_self"] = (lat, lat.copy())
    p["lattice_shifted"] = (lat + np.float32(1 / 16), lat)
    p["identical_targets"] = (np.concatenate([uniform(rng, 100), one[:3]]), one)
    p["coincident"] = (dup.copy(), dup)
    p["padded_targets"] = (uniform(rng, 300), padded)
    p["padded_queries"] = (padded, crop[::-1].copy())
    return p


TIES = _ties()


def test_zeros_and_ties(rg, oracle):
    names = list(TIES)
    case = Case.get("ties", rg, oracle, lambda: [TIES[k] for k in names], 6)
    got = case.run(rg)
    case.check(got, "ties")
    r = dict(zip(names, got))
    # every difference is exactly 0, of either sign with the weight's: +0 + (-0) = +0, so every component is +0.0f
    for k in ("lattice_self", "coincident"):
        assert (bits(r[k][0]) == 0).all() and (bits(r[k][1]) == 0).all(), k
    j = names.index("coincident")
    assert (case.g1[j] < 0).any() and (case.g1[j] > 0).any() and (case.g1[j] == 0).any()


# ---- 3. skipped indices ----
def test_skipped_indices(rg):
    rng = np.random.default_rng(9)
    a0, b0 = uniform(rng, 130), uniform(rng, 90)
    a0[7, 1] = np.nan
    b0[45, 2] = np.inf
    a1, b1 = clustered(rng, 200), uniform(rng, 150)
    a2, b2 = uniform(rng, 257), clustered(rng, 190)
    pairs = [(a0, b0), (a1, b1), (a2, b2)]
    i1, i2 = forward_indices(rg, pairs)
    assert (i1[0] == -1).all() and (i2[0] == -1).all()          # a non-finite coordinate on either side: the forward answers -1
    i1[1][[0, 5, 64, 199]] = [-1, 150, -1, 150]                 # by hand: -1 and m_j
    i2[1][[3, 149]] = [200, -1]                                 # ... and n_j
    g1, g2 = [weights(rng, len(a)) for a, _ in pairs], [weights(rng, len(b)) for _, b in pairs]
    got = backward(rg, pairs, g1, g2, i1, i2)
    for j, (a, b) in enumerate(pairs):
        same(got[j], R.pair_backward(a, b, g1[j], i1[j], g2[j], i2[j]), "pair %d vs the definition" % j)
    assert (bits(got[0][0]) == 0).all() and (bits(got[0][1]) == 0).all()          # rows with no term: +0.0f
    alone = backward(rg, pairs[2:], g1[2:], g2[2:], i1[2:], i2[2:])
    same(got[2], alone[0], "the clean pair against itself alone")


# ---- 4. determinism ----
def test_determinism(rg, oracle):
    torch = rg["torch"]
    case = Case.get("split24", rg, oracle, _split_pairs, 1)
    a = case.run(rg)
    b = case.run(rg)
    c = case.run(rg, stream=torch.cuda.Stream())
    d = case.run(rg, order=list(range(len(case.pairs)))[::-1])
    with arith(rg, 0):
        e0 = case.run(rg)
    with arith(rg, 1):
        e1 = case.run(rg)
    for j in range(len(case.pairs)):
        same(b[j], a[j], "second call, pair %d" % j)
        same(c[j], a[j], "side stream, pair %d" % j)
        same(d[j], a[j], "pairs in reverse order, pair %d" % j)
        same(e0[j], a[j], "genpc_set_arith(0), pair %d" % j)
        same(e1[j], a[j], "genpc_set_arith(1), pair %d" % j)


# ---- 5. against the existing backward ----
def test_against_the_rectangular_backward(rg, oracle):
    torch, ch = rg["torch"], rg["ch"]

    def make():
        rng = np.random.default_rng(12)
        return [(uniform(rng, n), uniform(rng, m)) for n, m in ((1000, 777), (65, 3000), (2049, 64), (300, 300), (1, 513), (4097, 1500))]
    case = Case.get("uniform6", rg, oracle, make, 13)
    got = case.run(rg)
    case.check(got, "uniform6")
    for j, (a, b) in enumerate(case.pairs):
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x[None])).cuda()      # noqa: E731
        gx1 = torch.zeros((1, len(a), 3), device="cuda")
        gx2 = torch.zeros((1, len(b), 3), device="cuda")
        assert ch.backward(t(a), t(b), gx1, gx2, t(case.g1[j]), t(case.g2[j]), t(case.i1[j]), t(case.i2[j])) == 1
        torch.cuda.synchronize()
        for side, ref in ((0, gx1), (1, gx2)):
            ref = ref.cpu().numpy()[0]
            print("pair %d gradxyz%d: max abs difference to genpc_chamfer_backward %.3g" % (j, side + 1, np.abs(got[j][side] - ref).max()))
            np.testing.assert_allclose(got[j][side], ref, rtol=1e-5, atol=1e-6)


# ---- 6. arguments ----
def test_bad_arguments_are_refused_and_write_nothing(rg):
    torch, lib, L = rg["torch"], rg["lib"], rg["L"]
    rng = np.random.default_rng(8)
    A, B = torch.from_numpy(uniform(rng, 20)).cuda(), torch.from_numpy(uniform(rng, 30)).cuda()
    G1, G2 = torch.from_numpy(weights(rng, 20)).cuda(), torch.from_numpy(weights(rng, 30)).cuda()
    I1, I2 = torch.zeros(20, dtype=torch.int32, device="cuda"), torch.zeros(30, dtype=torch.int32, device="cuda")
    o1 = torch.from_numpy(np.full((20, 3), POISON_F, np.float32)).cuda()
    o2 = torch.from_numpy(np.full((30, 3), POISON_F, np.float32)).cuda()
    good = [A, B, G1, I1, G2, I2, o1, o2]

    def call(c, noff, moff, null=None):
        na, ma = (ctypes.c_int * len(noff))(*noff), (ctypes.c_int * len(moff))(*moff)
        vp = lambda a: ctypes.cast(a, ctypes.c_void_p)      # noqa: E731
        p = [L.ptr(None if k == null else t) for k, t in enumerate(good)]
        return lib.genpc_chamfer_backward_ragged(c, None if null == "noff" else vp(na), p[0], None if null == "moff" else vp(ma), p[1],
                                                 p[2], p[3], p[4], p[5], p[6], p[7], L.stream_of(A))
    cases = [("a pair with xyz1 rows and no xyz2 rows", 2, [0, 10, 20], [0, 30, 30], None),
             ("a pair with xyz2 rows and no xyz1 rows", 2, [0, 20, 20], [0, 10, 30], None),
             ("only xyz2 has rows", 2, [0, 0, 0], [0, 10, 30], None),
             ("decreasing xyz1 offsets", 2, [0, 15, 10], [0, 10, 30], None),
             ("decreasing xyz2 offsets", 2, [0, 10, 20], [0, 20, 10], None),
             ("noff[0] != 0", 2, [5, 10, 20], [0, 10, 30], None),
             ("moff[0] != 0", 2, [0, 10, 20], [5, 10, 30], None),
             ("negative c", -1, [0, 10, 20], [0, 10, 30], None),
             ("too many pairs", 385, [0] * 386, [0] * 386, None),
             ("null noff", 2, [0, 10, 20], [0, 10, 30], "noff"),
             ("null moff", 2, [0, 10, 20], [0, 10, 30], "moff")]
    cases += [("null pointer %d" % k, 2, [0, 10, 20], [0, 10, 30], k) for k in range(8)]
    for what, c, noff, moff, null in cases:
        rc = call(c, noff, moff, null)
        assert rc == -1, what
        assert "genpc_chamfer_backward_ragged" in L.last_error(), what
    assert call(0, [0], [0]) == 1
    assert call(3, [0, 0, 0, 0], [0, 0, 0, 0]) == 1             # every pair empty on both sides
    torch.cuda.synchronize()
    assert (o1.cpu().numpy().view(np.uint32) == 0xDEADBEEF).all() and (o2.cpu().numpy().view(np.uint32) == 0xDEADBEEF).all()
    assert call(2, [0, 10, 20], [0, 10, 30]) == 1, L.last_error()          # (the same buffers are fine with good offsets)
    torch.cuda.synchronize()
    assert not (o1.cpu().numpy().view(np.uint32) == 0xDEADBEEF).any() and not (o2.cpu().numpy().view(np.uint32) == 0xDEADBEEF).any()


def test_backward_ragged_checks_buffers_against_offsets(rg):
    """chamfer_3D.backward_ragged: what only the binding can check -- dtypes, the buffers against the last offsets, host offsets."""
    torch, ch = rg["torch"], rg["ch"]
    f = lambda *s: torch.zeros(*s, device="cuda")                                     # noqa: E731
    i = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")                    # noqa: E731
    noff, moff = [0, 3, 8], [0, 4, 6]
    ok = dict(xyz1=f(8, 3), xyz2=f(6, 3), gradxyz1=f(8, 3), gradxyz2=f(6, 3), graddist1=f(8), graddist2=f(6), idx1=i(8), idx2=i(6))

    def call(noff=noff, moff=moff, **over):
        a = dict(ok, **over)
        return ch.backward_ragged(a["xyz1"], noff, a["xyz2"], moff, a["gradxyz1"], a["gradxyz2"], a["graddist1"], a["graddist2"], a["idx1"], a["idx2"])
    assert call() == 1
    for name, bad in (("xyz1", f(7, 3)), ("xyz2", f(6, 2)), ("gradxyz1", f(9, 3)), ("gradxyz2", f(5, 3)), ("graddist1", f(7)),
                      ("graddist2", f(8)), ("idx1", i(6)), ("idx2", i(8))):
        with pytest.raises(ValueError, match=name):
            call(**{name: bad})
    with pytest.raises(TypeError, match="idx1 must be torch.int32"):
        call(idx1=torch.zeros(8, dtype=torch.int64, device="cuda"))
    with pytest.raises(TypeError, match="graddist2 must be torch.float32"):
        call(graddist2=torch.zeros(6, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="differ in length"):
        call(moff=[0, 6])
    with pytest.raises(ValueError, match="lives on the host"):
        call(noff=torch.tensor(noff, device="cuda"))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        call(graddist1=torch.zeros(8))
