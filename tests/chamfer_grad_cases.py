"""The dense Chamfer backward (genpc_chamfer_backward, csrc/chamfer.hip) stated plainly, with the inputs that reach every path
of its two kernels.  tests/test_chamfer_grad_cases.py proves on the CPU that the cases reach what they say;
tests/test_gpu_chamfer_backward.py compares the kernels with `reference` on them.  Three parts.

  * `reference`: every term as the kernels state it, in float32 numpy (the same bits): g = fl(2 gd), d = fl(q - t),
    v = fl(g d); row q of the query's cloud gets init + v, row idx[q] of the other cloud gets -v, both directions, the sums in
    float64.  Beside the sums it returns, per output element, the number of scatter terms k and
    S = |init| + |own term| + sum |scatter terms|.
  * `bound(k, S)` = gamma(k + 2) S, gamma(j) = j u / (1 - j u), u = 2^-24: an fp32 sum of k + 2 numbers in ANY order is
    within gamma(k + 1) S of the exact sum (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2); one more j
    covers the float64 sum it is compared with.  Derived, not measured.
  * `census`: chamfer_grad_dir_kernel's branch selection per direction, tile, wave and trip, from the index arrays alone.

A CASE comes in two flavours.  `lattice`: integer coordinates, init a multiple of 1/2, gd from {1/4, 1/2, 3/4, 1}, so that
every term is a multiple of QUANTUM = 1/2 and, the coordinate range chosen from the fullest row, every partial sum of every
row in any order is an integer number of quanta below 2^24: exact in fp32, the result has no tolerance.  `float`: gen_pair
clouds, gd and init from rng.random.  The indices are the same in both flavours."""
import collections
import functools

import numpy as np

# csrc/chamfer.hip, csrc/common.h (tests/test_chamfer_grad_cases.py reads them from the code)
GRAD_TILE = 4096            # kGradTile: target rows a block owns
GRAD_LIST = 128             # kGradList: compacted hits a wave keeps per trip
GRAD_BLOCK = 1024           # kGradBlock
WAVE = 64                   # kWave
SLOTS = 8                   # entries a thread takes per trip
THRESHOLD = 262144          # points of both clouds from which a call takes chamfer_grad_dir_kernel

U = 2.0 ** -24
QUANTUM = 0.5
GD_LATTICE = np.array([0.25, 0.5, 0.75, 1.0], np.float32)

Case = collections.namedtuple("Case", "name flavour bsz n m xyz1 xyz2 gd1 gd2 idx1 idx2 init1 init2")


# ---------------------------------------------------------------------------------------------------------------------------
# The operation
def terms(q, t, gd, idx):
    """[b,nq,3] float32: v = fl(fl(2 gd) fl(q - t[idx])), each operation rounded once."""
    two = np.float32(2.0)
    g = (gd.astype(np.float32) * two).astype(np.float32)
    tt = np.take_along_axis(t, idx.astype(np.int64)[..., None], axis=1)
    d = (q - tt).astype(np.float32)
    v = (g[..., None] * d).astype(np.float32)
    assert g.dtype == np.float32 and d.dtype == np.float32 and v.dtype == np.float32
    return v


def reference(a, b, g1, g2, i1, i2, init1, init2):
    """-> (e1 [b,n,3], e2 [b,m,3]) float64, (k1 [b,n,1], k2 [b,m,1]) int64, (S1, S2) float64 shaped like e."""
    bsz, n, m = a.shape[0], a.shape[1], b.shape[1]
    v1, v2 = terms(a, b, g1, i1), terms(b, a, g2, i2)
    out = []
    for own, init, idx_in, v_in, rows in ((v1, init1, i2, v2, n), (v2, init2, i1, v1, m)):
        e = init.astype(np.float64) + own.astype(np.float64)
        S = np.abs(init.astype(np.float64)) + np.abs(own.astype(np.float64))
        k = np.zeros((bsz, rows), np.int64)
        flat = (np.arange(bsz, dtype=np.int64)[:, None] * rows + idx_in.astype(np.int64)).reshape(-1)
        e2, S2 = e.reshape(-1, 3), S.reshape(-1, 3)          # (views: add.at writes through)
        np.add.at(e2, flat, -v_in.astype(np.float64).reshape(-1, 3))
        np.add.at(S2, flat, np.abs(v_in.astype(np.float64)).reshape(-1, 3))
        np.add.at(k.reshape(-1), flat, 1)
        out.append((e, k[..., None], S))
    (e1, k1, S1), (e2, k2, S2) = out
    return (e1, e2), (k1, k2), (S1, S2)


def gamma(j):
    j = np.asarray(j, np.float64)
    return j * U / (1.0 - j * U)


def bound(k, S):
    return gamma(np.asarray(k, np.float64) + 2.0) * S


# ---------------------------------------------------------------------------------------------------------------------------
# The model of chamfer_grad_dir_kernel's control flow
def _census_dir(bsz, nq, nt, idx):
    """One launch: the queries' index array idx [bsz,nq] into nt target rows."""
    idx = np.asarray(idx, np.int64)
    assert idx.shape == (bsz, nq) and idx.min() >= 0 and idx.max() < nt         # (the kernels' premise: indices in range)
    tiles = -(-nt // GRAD_TILE)
    per_trip = SLOTS * GRAD_BLOCK
    trips = -(-nq // per_trip)                  # for (q0 = thread; q0 - thread < nq; q0 += 8 kGradBlock)
    waves = GRAD_BLOCK // WAVE
    q = np.arange(nq, dtype=np.int64)           # q = trip 8 kGradBlock + u kGradBlock + wave kWave + lane
    trip, r = q // per_trip, q % per_trip
    u, wave = r // GRAD_BLOCK, (r % GRAD_BLOCK) // WAVE
    tile = idx // GRAD_TILE                      # the one tile whose (unsigned)(I[q] - t0) < rows holds
    e = np.arange(bsz, dtype=np.int64)[:, None]
    key = ((((e * trips + trip[None]) * waves + wave[None]) * tiles + tile) * SLOTS + u[None]).reshape(-1)
    cnt = np.bincount(key, minlength=bsz * trips * waves * tiles * SLOTS).reshape(bsz, trips, waves, tiles, SLOTS)
    total = cnt.sum(-1)                          # [bsz, trips, waves, tiles]
    is_list = (total > 0) & (total <= GRAD_LIST)
    fed = cnt[is_list] > 0                       # [list trips, 8]
    hit = total.sum((0, 1, 2)) > 0               # [tiles]
    rows_last = nt - (tiles - 1) * GRAD_TILE
    return dict(
        queries=nq, targets=nt, tiles=tiles, trips=trips, rows_last=rows_last,
        tiles_hit=[int(t) for t in np.nonzero(hit)[0]],
        hits_past_first_tile=bool(hit[1:].any()),                       # a term lands at t0 > 0
        short_last_tile_hit=bool(rows_last < GRAD_TILE and hit[-1]),    # a hit tested against rows < kGradTile ...
        short_last_tile_past_first_hit=bool(rows_last < GRAD_TILE and tiles > 1 and hit[-1]),         # ... at t0 > 0
        one_row_tile_hit=bool(rows_last == 1 and hit[-1]),
        totals=set(int(t) for t in np.unique(total)),
        skip_trips=int((total == 0).sum()), list_trips=int(is_list.sum()), inplace_trips=int((total > GRAD_LIST).sum()),
        list_slots=set(int(s) for s in np.nonzero(fed.any(0))[0]) if fed.size else set(),
        list_slot_counts=set(int(c) for c in np.unique(fed.sum(1))) if fed.size else set(),
        tiles_per_wave_trip=int((total > 0).sum(-1).max()),          # over how many tiles one wave's 512 entries are spread
        max_row_terms=int(np.bincount((e * nt + idx).reshape(-1)).max()),
    )


def census(case):
    """What a call with the case's sizes and index arrays does; `case` needs bsz, n, m, idx1, idx2."""
    bsz, n, m = case.bsz, case.n, case.m
    out = dict(points=bsz * (n + m), kernel="tile" if bsz * (n + m) >= THRESHOLD else "atomic", decode=None, dirs=())
    if out["kernel"] == "atomic":
        # chamfer_grad_kernel: thread t < bsz n is direction 1's, the rest direction 2's
        out["directions_meet_in_a_wave"] = bool((bsz * n) % WAVE)
        return out
    out["decode"] = "xcd" if bsz % 8 == 0 else "plain"
    out["e_max"] = bsz - 1
    out["k_over_tiles_max"] = bsz // 8 - 1 if out["decode"] == "xcd" else None        # e = 8 (k / tiles) + xcd
    out["dirs"] = (_census_dir(bsz, n, m, case.idx1), _census_dir(bsz, m, n, case.idx2))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# The cases: name -> (bsz, n, m), the indices by name below
SHAPES = {
    "threshold": (1, 150001, 112143),
    "threshold_minus_1": (1, 150001, 112142),
    "batch3": (3, 50000, 40000),
    "batch8": (8, 20000, 13000),
    "batch16": (16, 10000, 6400),
    "list_boundary": (1, 253952, 8192),
    "few_queries": (1, 300, 261844),
    "single_query": (1, 1, 262143),
    "one_row_tile": (1, 4095, 258049),
    "crowded_last_row": (1, 258048, 4097),
    "small_1_1_1": (1, 1, 1),
    "small_2_1_700": (2, 1, 700),
    "small_2_700_1": (2, 700, 1),
    "small_5_257_255": (5, 257, 255),
}
SMALL = tuple(c for c in SHAPES if c.startswith("small_"))
TILE_CASES = tuple(c for c in SHAPES if c not in SMALL and c != "threshold_minus_1")
CASES = tuple(SHAPES)
FLOAT_CASES = tuple(c for c in CASES if c != "crowded_last_row")
OWN_ROW_CASES = ("threshold", "threshold_minus_1", "batch3", "batch16") + SMALL
_SEED = {c: 1000 + 10 * k for k, c in enumerate(SHAPES)}


@functools.lru_cache(maxsize=None)
def indices(name):
    """-> (idx1 [bsz,n] into m, idx2 [bsz,m] into n) int32, read-only: uniform over the other cloud unless the case says else."""
    bsz, n, m = SHAPES[name]
    rng = np.random.default_rng(_SEED[name])
    i1 = rng.integers(0, m, (bsz, n)).astype(np.int32)
    i2 = rng.integers(0, n, (bsz, m)).astype(np.int32)
    if name == "list_boundary":
        # in wave w of trip t the first 120 + (w + t) % 16 entries, slot-major, fall in tile 0 and the rest in tile 1
        q = np.arange(n)
        trip, r = q // (SLOTS * GRAD_BLOCK), q % (SLOTS * GRAD_BLOCK)
        u, wave, lane = r // GRAD_BLOCK, (r % GRAD_BLOCK) // WAVE, r % WAVE
        first = u * WAVE + lane < 120 + (wave + trip) % 16
        within = rng.integers(0, GRAD_TILE, n)
        i1 = np.where(first, within, GRAD_TILE + within).astype(np.int32)[None]
    elif name == "one_row_tile":
        i1[0, rng.choice(n, 200, replace=False)] = m - 1
    elif name == "crowded_last_row":
        i1[:] = m - 1
    for a in (i1, i2):
        a.setflags(write=False)
    return i1, i2


def lattice_range(name):
    """R: the lattice flavour's coordinates are integers of [-R, R] and init a multiple of QUANTUM of [-R, R].  A term is at
    most 2 gd |q - t| <= 4 R = 8 R quanta, so the fullest row (k scatter terms, its own and init) has
    S / QUANTUM <= (k + 1) 8 R + 2 R; R is the largest power of two up to 1024 that keeps this at or below 2^23."""
    bsz, n, m = SHAPES[name]
    i1, i2 = indices(name)
    k = max(int(np.bincount((np.arange(bsz)[:, None] * nt + i.astype(np.int64)).reshape(-1)).max())
            for i, nt in ((i1, m), (i2, n)))
    R = 1024
    while R > 1 and (k + 1) * 8 * R + 2 * R > 2 ** 23:
        R //= 2
    assert (k + 1) * 8 * R + 2 * R <= 2 ** 23, (name, k)
    return R


@functools.lru_cache(maxsize=2)
def case(name, flavour):
    """-> Case, read-only arrays."""
    bsz, n, m = SHAPES[name]
    i1, i2 = indices(name)
    rng = np.random.default_rng(_SEED[name] + (1 if flavour == "lattice" else 2))
    if flavour == "lattice":
        R = lattice_range(name)
        pts = lambda rows: rng.integers(-R, R + 1, (bsz, rows, 3)).astype(np.float32)
        a, b = pts(n), pts(m)
        g1, g2 = GD_LATTICE[rng.integers(0, 4, (bsz, n))], GD_LATTICE[rng.integers(0, 4, (bsz, m))]
        half = lambda rows: (rng.integers(-2 * R, 2 * R + 1, (bsz, rows, 3)) * QUANTUM).astype(np.float32)
        init1, init2 = half(n), half(m)
    elif flavour == "float":
        from conftest import gen_pair
        a, b = gen_pair(_SEED[name] + 3, (bsz, n, 3), (bsz, m, 3))
        g1, g2 = rng.random((bsz, n), dtype=np.float32), rng.random((bsz, m), dtype=np.float32)
        init1, init2 = rng.random((bsz, n, 3), dtype=np.float32), rng.random((bsz, m, 3), dtype=np.float32)
    else:
        raise KeyError(flavour)
    arrays = tuple(np.ascontiguousarray(x) for x in (a, b, g1, g2))
    inits = tuple(np.ascontiguousarray(x) for x in (init1, init2))
    for x in arrays + inits:
        x.setflags(write=False)
    return Case(name, flavour, bsz, n, m, *arrays, i1, i2, *inits)


@functools.lru_cache(maxsize=2)
def expected(name, flavour):
    """reference(...) of the case, computed once and shared: ((e1, e2), (k1, k2), (S1, S2)), read-only."""
    c = case(name, flavour)
    out = reference(c.xyz1, c.xyz2, c.gd1, c.gd2, c.idx1, c.idx2, c.init1, c.init2)
    for pair in out:
        for x in pair:
            x.setflags(write=False)
    return out


def old_large_call_inputs():
    """The sizes and index arrays of tests/test_gpu_chamfer.py::test_backward_large_call_forms, drawn as that test draws them."""
    rng = np.random.default_rng(77)
    bsz, n, m = 24, 9096, 3000
    rng.random((bsz, n, 3), dtype=np.float32)
    rng.random((bsz, m, 3), dtype=np.float32)
    i1 = rng.integers(0, m, (bsz, n)).astype(np.int32)
    i2 = rng.integers(0, 40, (bsz, m)).astype(np.int32)
    return Case("old_large_call", "float", bsz, n, m, None, None, None, None, i1, i2, None, None)
