"""Seeded input families for the tests that hold the oracle and the HIP library against the reference's own
kernels (tests/test_oracle_vs_reference.py, tests/test_gpu_reference_kernels.py) and for the script that
records the reference's results (tests/golden/make_reference_kernel_vectors.py).

TEST INFRASTRUCTURE ONLY.  Everything here is a pure function of its arguments, so that the CPU-side and the
GPU-side run of one seed see the same case.

The Chamfer shapes are chosen against the three code paths of NmDistanceKernel (chamfer3D.cu:28-124): a full
512-tile runs the unrolled body, a ragged tile runs a second unrolled body over end_k & ~3 targets and a
scalar tail over the rest; queries beyond 512 * 16 take the grid-stride loop, batch elements beyond 32 the
batch stride.
"""
import numpy as np

F = np.float32


def _pair(seed, b, n, m, shift=0.5):
    rng = np.random.default_rng(seed)
    return rng.random((b, n, 3), dtype=F) - F(shift), rng.random((b, m, 3), dtype=F) - F(shift)


# ------------------------------------------------------------------------------------------------------
# Chamfer
# ------------------------------------------------------------------------------------------------------
# shapes of tests/test_gpu_chamfer.py that a CPU affords (the 300-element batch is left to (40, 300, 64))
GPU_SUITE_SHAPES = [(1, 1, 1), (1, 63, 65), (2, 257, 31), (3, 1000, 4097), (1, 8192, 8192), (5, 300, 5000),
                    (64, 512, 640), (1, 1, 70001), (1, 70001, 1), (1, 255, 2049), (1, 2048, 2047), (1, 513, 33),
                    (2, 777, 4097), (1, 5000, 130), (3, 64, 64), (2, 700, 900), (40, 300, 64)]
# m % 512 in {0, 1, 2, 3, 4, 5, 511}, m < 4; n > 512 * 16; batch > 32
PATH_SHAPES = [(2, 300, 512), (1, 300, 1024), (2, 300, 513), (1, 300, 514), (1, 300, 515), (1, 300, 516),
               (2, 300, 517), (1, 300, 1029), (1, 300, 511), (1, 300, 1023), (1, 300, 1), (2, 300, 2),
               (1, 300, 3), (1, 8192 + 517, 517), (1, 2 * 8192 + 3, 5), (33, 70, 516), (67, 5, 1027)]

# target positions in a cloud of 1031 points (tiles [0,512) [512,1024) and a ragged tile of 7: an unrolled
# group 1024..1027 and a scalar tail 1028..1030) and of 1027 points (ragged tile of 3: scalar tail only)
NONFINITE_POSITIONS = [
    ("tile0_first", 1031, 0), ("later_tile_first", 1031, 512), ("group_pos1", 1031, 5), ("group_pos2", 1031, 6),
    ("group_pos3", 1031, 7), ("later_group_pos2", 1031, 512 + 10), ("group_first_not_tile_first", 1031, 8),
    ("ragged_tile_first", 1031, 1024), ("ragged_body", 1031, 1026), ("scalar_tail", 1031, 1029),
    ("tail_only_tile_first", 1027, 1024), ("tail_only_tile_last", 1027, 1026)]


# the same classes in the smallest clouds that have them (519 = one full tile and a ragged one of 7; 515: of 3), for
# the recorded fixture; "a later FULL tile" needs 1031
FIXTURE_POSITIONS = [
    ("tile0_first", 519, 0), ("group_pos2", 519, 6), ("group_first_not_tile_first", 519, 8),
    ("ragged_tile_first", 519, 512), ("ragged_body", 519, 514), ("scalar_tail", 519, 517),
    ("tail_only_tile_first", 515, 512), ("later_tile_first", 1031, 512)]


def chamfer_nonfinite_cases(n=96, values=("nan", "inf", "-inf"), positions=None):
    """One non-finite coordinate (or a whole non-finite point) at one position class per case.  Both directions are
    computed, so the second direction sees the same point as a QUERY."""
    out = []
    for vi, vname in enumerate(values):
        v = F(float(vname))
        for pi, (pname, m, pos) in enumerate(positions or NONFINITE_POSITIONS):
            a, b = _pair(1000 + 37 * vi + pi, 1, n, m)
            if (pi + vi) % 2:
                b[0, pos] = v                  # the whole point
            else:
                b[0, pos, (pi + vi) % 3] = v   # one coordinate
            out.append(("%s_%s" % (vname.replace("-", "neg"), pname), a, b))
        a, b = _pair(1900 + vi, 1, n, 1031 if positions is None else 519)
        a[0, 17, 1] = v                        # a query of the first direction
        out.append(("%s_query" % vname.replace("-", "neg"), a, b))
    if positions is not None:
        return out
    # several at once, opposite infinities (inf - inf = NaN distance) and a NaN-only tile
    a, b = _pair(1950, 2, n, 1031)
    b[0, 0, 0] = np.nan
    b[0, 512] = np.inf
    b[0, 1028, 2] = -np.inf
    a[0, 3] = np.inf
    a[0, 4] = -np.inf
    b[1, 512:1024] = np.nan
    a[1, 9, 0] = np.nan
    out.append(("mixed", a, b))
    return out


def chamfer_tie_cases():
    """Exact ties: integer lattices (inside a group of four, across groups, across tiles), duplicated halves, all
    points identical."""
    out = []
    rng = np.random.default_rng(12)
    for name, n, m, side in (("lattice6", 400, 1400, 6), ("lattice3", 300, 1031, 3), ("lattice2_small", 64, 7, 2)):
        g = rng.integers(0, side, size=(2, n + m, 3)).astype(F)
        out.append((name, g[:, :n].copy(), g[:, n:].copy()))
    a, b = _pair(5, 2, 700, 1030)
    b[:, 515:1030] = b[:, 0:515]               # every target twice, the copies in later tiles
    a[:, :100] = b[:, 200:300]                 # exact hits
    out.append(("duplicated_halves", a, b))
    a, b = _pair(6, 1, 200, 1031)
    b[0, 1:] = b[0, 3].copy()                  # all targets but the first are one point
    out.append(("one_value_after_first", a, b))
    z = np.zeros((2, 300, 3), F) + F(0.25)
    out.append(("all_identical", z, z[:, :77].copy()))
    out.append(("all_identical_tiles", z, np.zeros((2, 1031, 3), F) + F(0.25)))
    return out


def chamfer_scale_cases():
    out = []
    a, b = _pair(41, 1, 500, 1031)
    for scale, off_a, off_b in ((1e-18, 0.0, 0.0), (1e4, 0.0, 0.0), (1e12, 0.0, 0.0), (1.0, 1000.0, 1000.0),
                                (1.0, 0.0, 300.0), (1e-3, 5.0, 5.0)):
        out.append(("scale%g_off%g_%g" % (scale, off_a, off_b),
                    (a * F(scale) + F(off_a)).astype(F), (b * F(scale) + F(off_b)).astype(F)))
    return out


def chamfer_shape_cases(shapes):
    return [("uniform_%dx%dx%d" % s, *_pair(21 + i, *s)) for i, s in enumerate(shapes)]


def chamfer_fuzz_case(seed):
    """Random n, m, batch, scale, offset, duplicate share and NaN / inf sprinkling."""
    rng = np.random.default_rng(70000 + seed)
    b = int(rng.integers(1, 5)) if seed % 7 else int(rng.integers(33, 40))
    n = int(rng.integers(1, 3000)) if seed % 5 else int(rng.integers(8193, 9000))
    m = int(rng.integers(1, 2600))
    if b > 4:
        n, m = n % 200 + 1, m % 700 + 1
    scale = F(10.0 ** rng.uniform(-3, 3))
    off = F(rng.uniform(-1, 1) * 10.0 ** rng.uniform(-1, 2))
    x = (rng.random((b, n, 3), dtype=F) * scale + off).astype(F)
    y = (rng.random((b, m, 3), dtype=F) * scale + off * F(rng.integers(0, 2))).astype(F)
    dup = rng.uniform(0, 0.6) if seed % 2 else 0.0
    for c in (x, y):
        k = int(dup * c.shape[1])
        if k:
            c[:, rng.integers(0, c.shape[1], k)] = c[:, rng.integers(0, c.shape[1], k)]
    if seed % 3 == 0:
        for c in (x, y):
            for _ in range(int(rng.integers(1, 4))):
                v = (np.nan, np.inf, -np.inf)[int(rng.integers(0, 3))]
                c[int(rng.integers(0, b)), int(rng.integers(0, c.shape[1])), int(rng.integers(0, 3))] = v
    return x, y


# ------------------------------------------------------------------------------------------------------
# EMD
# ------------------------------------------------------------------------------------------------------
def emd_uniform(seed, b, n):
    rng = np.random.default_rng(seed)
    return rng.random((b, n, 3), dtype=F), rng.random((b, n, 3), dtype=F)


def emd_unnormalised(seed, b, n, scale, offset):
    x, y = emd_uniform(seed, b, n)
    return (x * F(scale) + F(offset)).astype(F), (y * F(scale) + F(offset)).astype(F)


def emd_duplicates(seed, b, n):
    """Every point drawn from n / 4 distinct ones (several exactly equal bids per bidder)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        base = rng.random((b, n // 4, 3), dtype=F)
        out.append(np.stack([base[i][rng.integers(0, n // 4, n)] for i in range(b)]))
    return out[0], out[1]


def emd_crowded(seed, b, n):
    """Hundreds of bidders on six objects and a knot of near-equal ones (tests/test_gpu_emd.py, crowded objects)."""
    rng = np.random.default_rng(seed)
    x = (rng.random((b, n, 3), dtype=F) * F(0.05)).astype(F)
    y = (rng.random((b, n, 3), dtype=F) + F(2.0)).astype(F)
    y[:, :6] = rng.random((b, 6, 3), dtype=F) * F(0.05) + F(0.1)
    y[b - 1, 6:40] = y[b - 1, 5] + rng.random((34, 3), dtype=F) * F(1e-4)
    return x, y


def emd_lattice(seed, b, n, side=9):
    """Integer lattice / side: masses of exactly equal bid values and increments of exactly eps.  Up to 2048 points
    (one tile of Bid) the thread partition scans in index order and names the first of equal objects, like a plain
    scan; from 2304 points on a thread scans its slice of tile 0 and then its slice of tile 1, and the partition
    decides (emd_cuda.cu:104-118, 136-139, 165-173)."""
    rng = np.random.default_rng(seed)
    return ((rng.integers(0, side, size=(b, n, 3)) / float(side)).astype(F),
            (rng.integers(0, side, size=(b, n, 3)) / float(side)).astype(F))


def emd_few_bidders(seed, n=2304, free=8):
    """Every bidder but `free` has an object at its own place: from the second round on fewer bidders remain than Bid
    has blocks (unass_per_block = 1, thread_per_unass = 256, most blocks idle; emd_cuda.cu:108-110)."""
    rng = np.random.default_rng(seed)
    x = rng.random((1, n, 3), dtype=F)
    y = x[:, rng.permutation(n)].copy()
    y[0, rng.choice(n, free, replace=False)] = rng.random((free, 3), dtype=F)
    return x, y


def emd_duplicate_pairs(seed, n=2304, pairs=40):
    """Uniform clouds in which `pairs` objects of the second 2048-tile are copies of objects of the first.  A bidder
    whose best object is such a pair sees two exactly equal bid values, and WHICH of the two it names is decided by
    the thread partition of Bid (emd_cuda.cu:104-118, 136-139, 165-173): from the second round on a thread scans its
    slice of tile 0 and then its slice of tile 1, and the merge keeps the lowest THREAD, not the lowest index."""
    rng = np.random.default_rng(seed)
    x, y = rng.random((1, n, 3), dtype=F), rng.random((1, n, 3), dtype=F)
    k1 = rng.choice(2048, pairs, replace=False)
    k2 = 2048 + rng.choice(n - 2048, pairs, replace=False)
    y[0, k2] = y[0, k1]
    return x, y


def emd_family_cases():
    """[(name, xyz1, xyz2, eps)]; every case is run for 1, 2, 3, 10 and 50 rounds."""
    c = []
    for i, n in enumerate((256, 512, 768, 1024, 2304)):
        c.append(("uniform_n%d" % n, *emd_uniform(300 + i, 1 + i % 3, n), 0.005))
    c.append(("uniform_n1024_eps002", *emd_uniform(310, 2, 1024), 0.002))
    c.append(("uniform_n2304_eps002", *emd_uniform(311, 1, 2304), 0.002))
    for scale, offset in ((100.0, 0.0), (30.0, 250.0), (1000.0, -500.0), (1e-3, 0.0)):
        c.append(("unnormalised_%g_%g" % (scale, offset), *emd_unnormalised(77, 2, 1024, scale, offset), 0.005))
    c.append(("duplicates_n512", *emd_duplicates(5, 3, 512), 0.005))
    c.append(("duplicates_n2304", *emd_duplicates(9, 1, 2304), 0.005))
    c.append(("crowded_n2048", *emd_crowded(59, 2, 2048), 0.005))
    c.append(("lattice_n256", *emd_lattice(20, 2, 256), 0.005))
    c.append(("lattice_n768", *emd_lattice(21, 1, 768), 0.005))
    c.append(("lattice_n1024_side4", *emd_lattice(22, 1, 1024, 4), 0.002))
    c.append(("lattice_n2304", *emd_lattice(23, 1, 2304, 12), 0.005))
    c.append(("duplicate_pairs_n2304", *emd_duplicate_pairs(638, 2304, 6), 0.005))
    return c


def emd_fuzz_case(seed, max_n=4096):
    """-> xyz1, xyz2, eps, iters.  Random n (multiples of 256 up to max_n), batch, eps and rounds; uniform, clustered
    or flattened clouds in general position, both clouds in one frame and at one scale.

    The family is chosen so that the reference itself is mostly determined.  GetMax picks the last writer among the
    bidders whose increment lies within 1e-6 of an object's largest, so every such near tie makes the result depend on
    the schedule.  Lattices and exact duplicates produce them in masses (increments of exactly eps), and so do
    bidders far outside the objects' cloud (best and second-best values nearly equal); those inputs are in
    emd_family_cases, where only the oracle's ascending convention is pinned.  General-position clouds still meet a
    near tie in about one case of five (see EMD_FUZZ_SEEDS)."""
    rng = np.random.default_rng(90000 + seed)
    n = 256 * int(rng.integers(1, max_n // 256 + 1))
    b = int(rng.integers(1, 4)) if n <= 2048 else 1
    iters = int(rng.integers(1, 51))
    eps = float(10.0 ** rng.uniform(-3, -1.7))
    kind = seed % 3
    scale = rng.uniform(0.3, 1.0)              # one scale and one frame for both clouds: bidders inside the objects' cloud
    centres = rng.random((b, 6, 3))

    def cloud():
        if kind == 0:
            x = rng.random((b, n, 3))
        elif kind == 1:
            x = np.stack([centres[i][rng.integers(0, 6, n)] for i in range(b)]) + 0.05 * rng.normal(size=(b, n, 3))
        else:
            x = rng.random((b, n, 3)) * np.array([1.0, 0.6, 0.3])
        return (x * scale).astype(F)
    return cloud(), cloud(), eps, iters


# The seeds of the EMD fuzz.  Exact and near ties inside GetMax's 1e-6 window are common enough that the reference
# itself is undetermined on about one case in five of this family (24 of the seeds 0..29 give the same dist and
# assignment under both schedules).  The list is SELECTED from the seeds 0..29 by that label, which only the reference
# decides: it keeps two of the six undetermined seeds (0 and 7) and 18 determined ones.
EMD_FUZZ_SEEDS = [0, 1, 3, 4, 5, 6, 7, 8, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 23]
CHAMFER_FUZZ_SEEDS = list(range(36))

def emd_fixture_cases():
    """[(name, xyz1, xyz2, eps, rounds)] recorded in tests/golden/ref_cuda_emd.npz: small, and schedule-independent in
    dist, assignment, bid and bid_increments, in both arithmetic modes.  What each is there for (every one was checked
    to fail against an oracle with that rule changed): the double-precision bid value shows in the last bits of
    bid_increments of every case past its first round; uniform_n1024_window flips assignments when GetMax's window is
    1e-5 instead of 1e-6; duplicate_pairs_n2304 names other objects when the bid partition is a plain scan."""
    return [("uniform_n256", *emd_uniform(300, 1, 256), 0.005, (1, 2, 3, 50)),
            ("uniform_n512_eps002", *emd_uniform(312, 1, 512), 0.002, (10,)),
            ("unnormalised_n512", *emd_unnormalised(78, 1, 512, 30.0, 250.0), 0.005, (3, 50)),
            ("crowded_n512", *emd_crowded(61, 1, 512), 0.005, (1,)),
            ("lattice_n256", *emd_lattice(20, 2, 256), 0.005, (1,)),
            ("uniform_n1024_window", *emd_uniform(504, 1, 1024), 0.005, (20,)),
            ("duplicate_pairs_n2304", *emd_duplicate_pairs(638, 2304, 6), 0.005, (2,))]


def emd_schedule_independent(O, x, y, eps, iters, fma_mode=0):
    """-> (dist, assignment under the ascending schedule, whether the descending schedule gives the same two)."""
    d0, a0 = O.ref_emd_forward(x, y, eps, iters, fma_mode, 0)
    d1, a1 = O.ref_emd_forward(x, y, eps, iters, fma_mode, 1)
    return d0, a0, same_bits(d0, d1) and same_bits(a0, a1)


RECORDED = ("dist", "assignment", "bid", "bid_increments")


def emd_recorded_outputs(O, x, y, eps, iters, fma_mode=0):
    """-> ({dist, assignment, bid, bid_increments} under the ascending schedule, whether the descending schedule gives
    the same four).  bid and bid_increments are those of the last round; they show the bid arithmetic and the thread
    partition directly, where dist and assignment show them only once an assignment flips."""
    s0 = O.ref_emd_forward(x, y, eps, iters, fma_mode, 0, return_state=True)[2]
    s1 = O.ref_emd_forward(x, y, eps, iters, fma_mode, 1, return_state=True)[2]
    return {k: s0[k] for k in RECORDED}, all(same_bits(s0[k], s1[k]) for k in RECORDED)


def same_bits(a, b):
    """Bit-for-bit equality of two arrays (NaN payloads and signed zeros included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
