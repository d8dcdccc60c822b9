"""The inputs of one step of the loop's seeded nearest-neighbour search (csrc/nn_seeded.hip through genpc_nn_seeded_step):
clouds, poses and seed policies, all from fixed rng seeds.  tests/test_nn_seeded_cases.py proves on the CPU that they have the
properties tests/test_gpu_nn_seeded.py relies on (ties, duplicates, finite posed points, which grid sizes are reached); the GPU
tests compare the kernel with oracle.chamfer_forward on the posed cloud the GPU returned, bit for bit.

A CASE is (rest [b,nm,3], center [b,3], params [b,10], stat [b,ns,3]), float32: the static cloud of every cloud family but
`lattice` is made FROM the pose -- another sampling of the same shape, posed with the oracle's transform, its front half (z at
or above the median) -- so that the two clouds of a step overlap as they do in the loop, whatever the pose.

`interior` (lattice): a query that lies strictly inside the targets' bounding box on at least two of the three axes.  Such a
query of the 9 x 9 x 9 lattice has 4 (on a face) or 8 equidistant cell centres, every cell centre has 8 equidistant lattice
points; only the edges and corners of the lattice (92 of 729 points) have fewer than 4.  (With `strictly inside on all three
axes' direction 1 would have 343 of 729 interior queries, less than half: the 7 x 7 x 7 inner lattice.)"""
import functools

import numpy as np

INT_MIN = -2 ** 31
QUERIES_PER_BLOCK = 64            # nn_seeded.hip: kBlock / kSLPQ

IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 0, 0], np.float32)


def _oracle():
    from oracle import oracle
    oracle.build()
    return oracle


def rot(axis, deg):
    """Rodrigues, float64."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


# ---------------------------------------------------------------------------------------------------------------------------
# Poses: name -> params[10] for a cloud `size` across.  rotation_6d_to_matrix takes the first two ROWS of R.
# (translation_1e6 is not one of the loop's regimes: it is there because it is the one pose that needs the moving grid's margins.)
R_LOOP = rot([0.3, 1.0, 0.2], 11.0)
R_170 = rot([1.0, 2.0, 3.0], 170.0)
LOG_S_LOOP = float(np.log(0.9))
GIVE_UP = ("parallel", "a1_zero", "ls_plus50", "ls_minus50")        # poses for which the kernel must stop culling
POSES = ("identity", "loop", "rot170", "ls_plus2", "ls_minus2", "unnormalised", "far_translation", "translation_1e6") + GIVE_UP


def pose(name, size):
    p = np.zeros(10)
    p[0:3], p[3:6] = R_LOOP[0], R_LOOP[1]
    p[6:9] = 0.02 * size * np.array([1.0, -0.5, 0.25])
    p[9] = LOG_S_LOOP
    if name == "identity":
        p[:] = IDENTITY
    elif name == "loop":
        pass
    elif name == "rot170":
        p[0:3], p[3:6] = R_170[0], R_170[1]
    elif name == "ls_plus2":
        p[9] = 2.0
    elif name == "ls_minus2":
        p[9] = -2.0
    elif name == "unnormalised":          # a1 of length 5, a2 (length 2) at 60 degrees to it: what Adam makes of a rotation at once
        p[0:3] = 5.0 * R_LOOP[0]
        p[3:6] = 2.0 * (np.cos(np.pi / 3) * R_LOOP[0] + np.sin(np.pi / 3) * R_LOOP[1])
    elif name == "far_translation":
        p[6:9] = 50.0 * size * np.array([0.6, -0.64, 0.48])
    elif name == "translation_1e6":
        # 1e6 sizes from the centre an ulp is 1 / 30 ... 1 / 15 of the cloud: the posed points collapse onto that lattice (many
        # distances are exactly 0 and tie) and a static point brought back to the rest frame is off by as much -- the pose at
        # which the search depends on its absolute margin (`mag`: without it, nn_seeded_kernel answers these ties wrongly)
        p[6:9] = 1e6 * size * np.array([0.6, -0.64, 0.48])
    elif name == "parallel":
        p[3:6] = 2.0 * p[0:3]
    elif name == "a1_zero":
        p[0:3] = 0.0
    elif name == "ls_plus50":
        p[9] = 50.0
    elif name == "ls_minus50":
        p[9] = -50.0
    else:
        raise KeyError(name)
    return p.astype(np.float32)


def moved(params, by=0.01):
    """The pose moved by `by` in every parameter: one Adam step of the loop at lr = by (its first step moves every parameter by lr)."""
    return (np.asarray(params, np.float32) + np.float32(by)).astype(np.float32)


def posed_by_oracle(rest, center, params):
    """[b,nm,3] -> the oracle's transform, element by element: the CPU tests' stand-in for what the GPU returns (equal to 3e-7)."""
    o = _oracle()
    return np.stack([o.pose_transform(rest[e], center[e], params[e]) for e in range(rest.shape[0])])


# ---------------------------------------------------------------------------------------------------------------------------
# Clouds
def _ellipsoid_points(rng, n):
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (u * np.array([0.5, 0.3, 0.2])).astype(np.float32)


def _front_half(rest_like, center, params, ns):
    """ns of the points of `rest_like` posed by the oracle whose z is at or above the median (at least half of them are)."""
    p = _oracle().pose_transform(rest_like, center, params)
    keep = p[p[:, 2] >= np.median(p[:, 2])]
    assert keep.shape[0] >= ns, (keep.shape, ns)
    return np.ascontiguousarray(keep[:ns])


def _finish(rest, params, stat_from, ns, center=None):
    rest = np.ascontiguousarray(rest, np.float32)
    center = rest.astype(np.float64).mean(0).astype(np.float32) if center is None else np.asarray(center, np.float32)
    stat = _front_half(stat_from, center, params, ns)
    return rest[None], center[None], np.asarray(params, np.float32)[None], stat[None]


def size_of(rest):
    r = np.asarray(rest, np.float64).reshape(-1, 3)
    return float(max((r.max(0) - r.min(0)).max(), 1e-30))


def _shaped(seed, nm, ns, shape=lambda x: x, scale=1.0, shift=(0.0, 0.0, 0.0)):
    """(rest, another sampling 2 ns + 8 points strong) of the ellipsoid, flattened / scaled / shifted"""
    rng = np.random.default_rng(seed)
    f = lambda x: (shape(x.astype(np.float64)) * scale + np.asarray(shift, np.float64)).astype(np.float32)
    return f(_ellipsoid_points(rng, nm)), f(_ellipsoid_points(rng, 2 * ns + 8))


def _flat(x):
    x = x.copy(); x[:, 2] = 0.125
    return x


def _line(x):
    x = x.copy(); x[:, 1] = -0.25; x[:, 2] = 0.125
    return x


def _point(x):
    x = x.copy(); x[:] = (0.25, -0.25, 0.125)
    return x


# name -> (seed, nm, ns, keyword arguments of _shaped)
_FAMILY = {
    "ellipsoid": (11, 1000, 777, {}),
    "ellipsoid65": (12, 65, 63, {}),
    "ellipsoid1100": (13, 1100, 777, {}),       # 18 blocks of 64 queries: the sampled launch's sizes
    "tiny_1_1": (21, 1, 1, {}), "tiny_1_5": (22, 1, 5, {}), "tiny_5_1": (23, 5, 1, {}), "tiny_7_3": (24, 7, 3, {}),
    "flat": (31, 1000, 777, dict(shape=_flat)),
    "line": (32, 1000, 777, dict(shape=_line)),
    "point": (33, 300, 200, dict(shape=_point)),
    "far_origin": (41, 1000, 777, dict(shift=(1000.0, -2000.0, 500.0))),
    "scale_1e-3": (51, 1000, 777, dict(scale=1e-3)),
    "scale_1e3": (52, 1000, 777, dict(scale=1e3)),
}
CAP_NM, CAP_NS = 24001, 23111
POSED_CLOUDS = tuple(_FAMILY) + ("duplicates", "cap", "batch3")          # every cloud but `lattice`: run with every pose
ALL_POLICY_CLOUDS = ("ellipsoid", "ellipsoid65", "duplicates", "batch3")  # (and lattice): run with every seed policy
BATCH3_POSES = ("loop", "rot170", "ls_minus2")


def _rest_of(cloud):
    """(rest [nm,3], the other sampling the static cloud is cut from, ns)"""
    if cloud in _FAMILY:
        seed, nm, ns, kw = _FAMILY[cloud]
        rest, other = _shaped(seed, nm, ns, **kw)
        return rest, other, ns
    if cloud == "duplicates":
        rest, other = _shaped(11, 1000, 777)
        rng = np.random.default_rng(61)
        return np.ascontiguousarray(rest[rng.integers(0, 1000, 1000)]), other, 777
    if cloud == "cap":
        rng = np.random.default_rng(71)
        box = lambda n: ((rng.random((n, 3)) - 0.5) * np.array([1.0, 0.8, 0.6])).astype(np.float32)
        return box(CAP_NM), box(2 * CAP_NS + 8), CAP_NS
    raise KeyError(cloud)


@functools.lru_cache(maxsize=None)
def case(cloud, pose_name):
    """-> (rest [b,nm,3], center [b,3], params [b,10], stat [b,ns,3]); read-only arrays, made once per process."""
    if cloud == "lattice":
        assert pose_name == "lattice"
        out = lattice()[:4]
    elif cloud == "batch3":
        # three ellipsoid elements, each with its own sampling, pose and centre (the mean moved off by a different amount);
        # pose_name is the pose of element 0, the other two take BATCH3_POSES[1:]
        parts = []
        for e, pn in enumerate((pose_name,) + BATCH3_POSES[1:]):
            rest, other = _shaped(81 + e, 1000, 777)
            c = rest.astype(np.float64).mean(0) + 0.05 * e * np.array([1.0, -1.0, 0.5])
            parts.append(_finish(rest, pose(pn, size_of(rest)), other, 777, center=c))
        out = tuple(np.concatenate([p[k] for p in parts]) for k in range(4))
    else:
        rest, other, ns = _rest_of(cloud)
        out = _finish(rest, pose(pose_name, size_of(rest)), other, ns)
        if cloud == "duplicates":          # padded to 1024 by repeating its first points
            stat = out[3][0]
            out = out[:3] + (np.ascontiguousarray(np.concatenate([stat, stat[:1024 - 777]]))[None],)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def lattice():
    """-> (rest, center, params, stat, the posed cloud as it must come out [1,729,3]).  The 9 x 9 x 9 integer lattice in
    shuffled order turned by exactly 90 degrees about z through the integer point (4, 4, 4): (x, y, z) -> (y, 8 - x, z), every
    operation of the transform exact in fp32; against the 8 x 8 x 8 cell centres in shuffled order."""
    rng = np.random.default_rng(91)
    g = np.arange(9, dtype=np.float32)
    rest = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[rng.permutation(729)]
    c = np.arange(8, dtype=np.float32) + 0.5
    stat = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)[rng.permutation(512)]
    center = np.array([4, 4, 4], np.float32)
    params = np.array([0, 1, 0, -1, 0, 0, 0, 0, 0, 0], np.float32)
    expect = np.stack([rest[:, 1], 8.0 - rest[:, 0], rest[:, 2]], -1).astype(np.float32)
    out = (np.ascontiguousarray(rest)[None], center[None], params[None], np.ascontiguousarray(stat)[None], expect[None])
    for a in out:
        a.setflags(write=False)
    return out


def interior(queries, targets):
    """[nq] bool: strictly inside the targets' bounding box on at least two axes (the module docstring)."""
    lo, hi = targets.min(0), targets.max(0)
    return ((queries > lo) & (queries < hi)).sum(1) >= 2


# ---------------------------------------------------------------------------------------------------------------------------
# Answers and seeds
def answers(oracle, posed, stat, mode):
    """oracle.chamfer_forward on a batch -> (d1, i1, d2, i2)."""
    d1, d2, i1, i2 = oracle.chamfer_forward(posed, stat, mode)
    return d1, i1, d2, i2


def highest_minima(oracle, posed, stat, mode):
    """-> (h1 [b,nm], h2 [b,ns]): for every query the HIGHEST index among its bit-equal nearest targets -- the oracle run
    against the targets in reversed order returns the first of them in that order.  A query whose two answers differ has a tie."""
    _, r1, _, _ = answers(oracle, posed, np.ascontiguousarray(stat[:, ::-1]), mode)
    _, _, _, r2 = answers(oracle, np.ascontiguousarray(posed[:, ::-1]), stat, mode)
    return (stat.shape[1] - 1 - r1).astype(np.int32), (posed.shape[1] - 1 - r2).astype(np.int32)


def farthest(queries, targets):
    """[b,nq] int32: the index of the target farthest from every query (float64, first of equals)."""
    out = np.empty(queries.shape[:2], np.int32)
    for e in range(queries.shape[0]):
        q, t = queries[e].astype(np.float64), targets[e].astype(np.float64)
        d = (q * q).sum(1)[:, None] - 2.0 * q @ t.T + (t * t).sum(1)[None]
        out[e] = np.argmax(d, 1)
    return out


POLICIES = ("none", "out_of_range", "exact", "farthest", "random", "previous_step", "tie_high")
CHEAP_POLICIES = ("exact", "none")           # what the clouds outside ALL_POLICY_CLOUDS are run with


def seeds(policy, oracle, posed, stat, mode, rest=None, center=None, params=None, exact=None):
    """-> (seed1 [b,nm], seed2 [b,ns]) int32 for the step whose posed cloud is `posed` (the GPU's, or the oracle's stand-in).
    exact = answers(...) of that step where the caller has them already.  previous_step needs rest, center, params."""
    b, nm, ns = posed.shape[0], posed.shape[1], stat.shape[1]
    shapes = ((b, nm), (b, ns))
    counts = (ns, nm)
    if policy == "none":
        return tuple(np.full(s, -1, np.int32) for s in shapes)
    if policy == "out_of_range":
        out = []
        for s, nt in zip(shapes, counts):
            k = np.arange(s[0] * s[1]).reshape(s) % 3
            out.append(np.where(k == 0, nt, np.where(k == 1, nt + 7, INT_MIN)).astype(np.int32))
        return tuple(out)
    if policy == "exact":
        _, i1, _, i2 = exact if exact is not None else answers(oracle, posed, stat, mode)
        return i1.astype(np.int32), i2.astype(np.int32)
    if policy == "farthest":
        return farthest(posed, stat), farthest(stat, posed)
    if policy == "random":
        rng = np.random.default_rng(101)
        return tuple(rng.integers(0, nt, s).astype(np.int32) for s, nt in zip(shapes, counts))
    if policy == "previous_step":
        before = posed_by_oracle(rest, center, np.stack([moved(p) for p in params]))
        _, i1, _, i2 = answers(oracle, before, stat, mode)
        return i1.astype(np.int32), i2.astype(np.int32)
    if policy == "tie_high":
        return highest_minima(oracle, posed, stat, mode)
    raise KeyError(policy)


def sampled_mask(b, nq, block_begin, sample):
    """[b,nq] bool: the queries a launch with `sample` answers -- those of the blocks whose number (block_begin + element *
    blocks per element + block inside the element) is a multiple of `sample`; also the number of blocks of the direction."""
    per = -(-nq // QUERIES_PER_BLOCK)
    blk = block_begin + np.arange(b)[:, None] * per + np.arange(nq)[None, :] // QUERIES_PER_BLOCK
    return blk % sample == 0, b * per
