"""The inputs of the tests of the sampling check (csrc/fps_verify.hip: fps_verify_kernel, through genpc_fps_verify_probe): small
clouds, their right sampling sequences and MUTANTS of them, each wrong in one step and nowhere else, all from fixed rng seeds.
tests/test_fps_check_definition.py proves on the CPU that they are what tests/test_gpu_fps_check.py takes them for: every right
sequence passes oracle.fps_check, every mutant's first wrong step is the mutated one, every (kind, position class) pair below
has a case and the witnesses of kinds 3 and 4 include the points named in WITNESS_POINTS.  The reference alone decides what a
case is: `expect` is oracle.fps_check's answer, never the GPU's.

A CASE is a dict: cloud (name), mode (arithmetic), k, kind (0: a right sequence, 1 .. 9: below), j (the mutated step, -1 for
kind 0), cls (the position classes of j), idx[k] int32, minima[k] float32 (minima[0] = +inf), witness (kinds 3, 4: the points that
show the error), expect (the first wrong step by the definition, -1: none).

Kinds.  1: M_j one ulp lower.  2: M_j one ulp higher (only the sample itself shows it).  3: the point with the largest running
minimum BELOW the arg-max's, recorded with its own running minimum (a self-consistent step; only the true arg-max shows it).
4: at a step with several arg-maxima the second of them, M_j unchanged (only the index rule shows it, at the first arg-max
alone).  5: steps j and j + 1 exchanged with their minima (a sample drawn a step early).  6: an earlier sample again, M_j
unchanged.  7: idx[j] = n, -1, INT_MIN.  8: idx[0] = 1.  9: k = 1 with idx[0] = 3.

Position classes of a step j of a k-sample sequence (kinds 1 .. 6): `trip` 1, 7, 8, 9 (round a trip of eight samples of the
kernel's inner loop); `seg<nseg>` per - 1, per, per + 1 for nseg = 1, 2, 3, 16 segments, per as the kernel computes it (sample
j - 1 decides step j: step per is the last of segment 0, step per + 1 the first of segment 1); `tile` 1023, 1024, 1025 (the
kernel stages 1024 samples at a time); `tail` k - 2, k - 1 (the loop behind the trips of eight, the last step)."""
import functools

import numpy as np

INT_MIN = -2 ** 31
TILE = 1024                       # fps_verify.hip: kFVTile
BLOCK = 128                       # fps_plan.h: kFVBlock
MAX_SEG = 16                      # fps_plan.h: kFVMaxSeg
FORCED_NSEG = (1, 2, 3, 16)
NSEGS = (0,) + FORCED_NSEG        # 0: as many segments as production takes
CLASSES = ("trip",) + tuple("seg%d" % s for s in FORCED_NSEG) + ("tile", "tail")
POSITION_KINDS = (1, 2, 3, 4, 5, 6)
WITNESS_POINTS = ("0", "127", "128", "n-1")       # n - 1 of a cloud whose size is no multiple of BLOCK: the padding lanes repeat it

UNIFORM = (1, 2, 9, 127, 128, 129, 1000, 1300)
LATTICE_SEED = 8
DUPS_N, DUPS_REPEATED = 297, 40   # (k - 1 = 296 is a multiple of 8: the last steps are at the one-segment cut as well)


def _oracle():
    from oracle import oracle
    oracle.build()
    return oracle


def per_of(k, nseg):
    """Samples per segment, as fps_verify_kernel computes it."""
    return (((k - 1) + nseg - 1) // nseg + 7) & ~7


@functools.lru_cache(maxsize=None)
def clouds():
    """name -> [n,3] float32 (read-only)."""
    out = {}
    for n in UNIFORM:
        rng = np.random.default_rng(1000 + n)
        out["uniform%d" % n] = rng.random((n, 3), dtype=np.float32) - np.float32(0.5)
    # lattices: distances are exact in fp32, many steps have several arg-maxima (8^3; 11^3, which has steps beyond the tile)
    for side, name in ((8, "lattice512"), (11, "lattice1331")):
        rng = np.random.default_rng(LATTICE_SEED + side)
        g = np.arange(side, dtype=np.float32) / np.float32(8 if side == 8 else 16)
        lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        out[name] = lat[rng.permutation(len(lat))].copy()
    rng = np.random.default_rng(40)
    d = rng.random((DUPS_N, 3), dtype=np.float32) - np.float32(0.5)
    d[DUPS_N - DUPS_REPEATED:] = d[:DUPS_REPEATED]          # the running minima are 0 for the last 40 steps of k = n
    out["dups%d" % DUPS_N] = d
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def right(cloud, mode, k):
    """The right sequence: oracle.fps_minima -> (idx[k], minima[k]), read-only."""
    idx, minima = _oracle().fps_minima(clouds()[cloud], k, mode)
    idx.setflags(write=False)
    minima.setflags(write=False)
    return idx, minima


@functools.lru_cache(maxsize=256)
def running(cloud, mode, k, j):
    """The running minima of all points after samples 0 .. j - 1 of the right sequence (j >= 1): the minimum over those samples
    of the oracle's squared distance of the mode."""
    x = clouds()[cloud]
    idx, _ = right(cloud, mode, k)
    d1 = _oracle().chamfer_forward(x[None], x[idx[:j]][None], mode)[0]
    return d1[0]


def positions(k):
    """step j -> set of position classes, for the steps 1 <= j <= k - 1 that are in a class."""
    pos = {}

    def add(j, cls):
        if 1 <= j <= k - 1:
            pos.setdefault(j, set()).add(cls)
    for j in (1, 7, 8, 9):
        add(j, "trip")
    for nseg in FORCED_NSEG:
        per = per_of(k, nseg)
        for j in (per - 1, per, per + 1):
            add(j, "seg%d" % nseg)
    for j in (TILE - 1, TILE, TILE + 1):
        add(j, "tile")
    for j in (k - 2, k - 1):
        add(j, "tail")
    return pos


def mutate(cloud, mode, k, kind, j, value=None):
    """(idx, minima, witness) of the right sequence made wrong in step j alone, or None where the step does not offer the kind."""
    n = len(clouds()[cloud])
    ridx, rmin = right(cloud, mode, k)
    idx, minima = ridx.copy(), rmin.copy()
    witness = None
    if kind == 1:
        minima[j] = np.nextafter(rmin[j], np.float32(-np.inf), dtype=np.float32)
    elif kind == 2:
        minima[j] = np.nextafter(rmin[j], np.float32(np.inf), dtype=np.float32)
    elif kind == 3:
        D = running(cloud, mode, k, j)
        below = D < rmin[j]
        if not below.any():
            return None
        v = D[below].max()
        idx[j] = int(np.flatnonzero(D == v)[0])
        minima[j] = v
        witness = np.flatnonzero(D > v)
    elif kind == 4:
        ties = np.flatnonzero(running(cloud, mode, k, j) == rmin[j])
        if len(ties) < 2:
            return None
        assert ties[0] == ridx[j]
        idx[j] = int(ties[1])
        witness = ties[:1]
    elif kind == 5:
        if j + 1 > k - 1:
            return None
        idx[j], idx[j + 1] = ridx[j + 1], ridx[j]
        minima[j], minima[j + 1] = rmin[j + 1], rmin[j]
    elif kind == 6:
        earlier = [e for e in range(j - 1, -1, -1) if ridx[e] != ridx[j]]
        if not earlier:
            return None
        idx[j] = ridx[earlier[len(earlier) // 2]]
    elif kind == 7:
        idx[j] = value
    elif kind == 8:
        if n < 2:
            return None
        idx[0] = 1
    elif kind == 9:
        idx[0] = 3
    else:
        raise ValueError(kind)
    if np.array_equal(idx, ridx) and np.array_equal(minima[1:], rmin[1:]):
        return None          # (exchanging two equal steps: not a mutant)
    return idx, minima, witness


def _case(cloud, mode, k, kind, j, cls, idx, minima, witness):
    expect = _oracle().fps_check(clouds()[cloud], idx, minima, mode)
    return dict(cloud=cloud, mode=mode, k=k, kind=kind, j=j, cls=frozenset(cls), idx=idx, minima=minima,
                witness=None if witness is None else tuple(int(w) for w in witness), expect=expect)


def witness_steps(cloud, mode, k):
    """Steps whose sample is point 127, 128 or n - 1 (n no multiple of BLOCK): kind 3's witnesses there."""
    n = len(clouds()[cloud])
    want = {127, 128} | ({n - 1} if n % BLOCK else set())
    idx, _ = right(cloud, mode, k)
    return [j for j in range(1, k) if int(idx[j]) in want]


@functools.lru_cache(maxsize=None)
def cases(mode):
    """Every case of one arithmetic mode: the right sequences (k = n and k = 1 of every cloud), then the mutants."""
    out = []
    for cloud, x in clouds().items():
        n = len(x)
        for k in sorted({n, 1}):
            idx, minima = right(cloud, mode, k)
            out.append(_case(cloud, mode, k, 0, -1, (), idx, minima, None))
    for cloud, x in clouds().items():
        n = k = len(x)
        pos = positions(k)
        for kind in POSITION_KINDS:
            if kind == 4 and not (cloud.startswith("lattice") or cloud.startswith("dups")):
                continue          # (exact ties: the lattices, and the repeated points' zeros)
            for j in sorted(pos):
                m = mutate(cloud, mode, k, kind, j)
                if m is not None:
                    out.append(_case(cloud, mode, k, kind, j, pos[j], *m))
        for j in witness_steps(cloud, mode, k):
            m = mutate(cloud, mode, k, 3, j)
            if m is not None:
                out.append(_case(cloud, mode, k, 3, j, pos.get(j, ()), *m))
        # kind 7: the first step, a segment cut, the tile, the last step
        for j in sorted({1, per_of(k, 2), per_of(k, 2) + 1, TILE, k - 1}):
            if 1 <= j <= k - 1:
                for value in (n, -1, INT_MIN):
                    out.append(_case(cloud, mode, k, 7, j, pos.get(j, ()), *mutate(cloud, mode, k, 7, j, value)))
        m = mutate(cloud, mode, k, 8, 0)
        if m is not None:
            out.append(_case(cloud, mode, k, 8, 0, (), *m))
        if n >= 4:
            out.append(_case(cloud, mode, 1, 9, 0, (), *mutate(cloud, mode, 1, 9, 0)))
    return out


# The job tables: eight clouds of different n and k in one call; (cloud, k, the kind of the slot's mutant)
TABLE = (("uniform9", 9, 3), ("uniform127", 100, 1), ("uniform128", 128, 2), ("uniform129", 64, 5), ("uniform1000", 300, 6),
         ("lattice512", 512, 4), ("dups%d" % DUPS_N, DUPS_N, 4), ("uniform1300", 1300, 3))
TABLE_NSEG = (1, 3)


@functools.lru_cache(maxsize=None)
def tables(mode):
    """Nine job tables (lists of eight cases): all right, then the mutant in slot q = 0 .. 7 and the other seven right."""
    good = []
    bad = []
    for cloud, k, kind in TABLE:
        idx, minima = right(cloud, mode, k)
        good.append(_case(cloud, mode, k, 0, -1, (), idx, minima, None))
        steps = sorted(range(1, k), key=lambda j: (abs(j - k // 2), j))          # the step nearest the middle that offers the kind
        if kind == 4 and cloud.startswith("dups"):
            steps = steps[::-1]                                                  # (its ties are the zeros of the last steps)
        for j in steps:
            m = mutate(cloud, mode, k, kind, j)
            if m is not None:
                bad.append(_case(cloud, mode, k, kind, j, (), *m))
                break
        else:
            raise AssertionError("no step of %s offers kind %d" % (cloud, kind))
    return [list(good)] + [[bad[q] if s == q else good[s] for s in range(len(TABLE))] for q in range(len(TABLE))]
