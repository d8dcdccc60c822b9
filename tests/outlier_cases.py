"""The clouds of the ragged outlier-filter tests (test_outlier_ragged_host.py, test_gpu_knn_mean_ragged.py,
test_gpu_outlier_ragged.py, test_gpu_fuse_scans.py) and the filter's statistics restated in numpy, in the summation order
include/genpc_hip.h defines.  No tests here.

The sizes: 1, 5 and 21 -- at or around fewer points than k, short lists; 63 / 64 / 65 and 255 / 256 / 257 -- the edges of a wave
and of a work item of the search; 8193 -- where the single call's build changes its number of pieces; lattice and identical300
-- exact ties at the k-th place and zero extent; plane -- an inactive axis; cluster_far -- empty cells; offset_1e3 and scale_1e-2
-- the grid's slack at other magnitudes; an empty cloud; a NaN and an infinite coordinate, in the MIDDLE of the batch so that
their neighbours prove the isolation.  The draws are order-dependent: the margins test_outlier_ragged_host.py asserts were
checked for exactly this generator."""
import numpy as np


def _clouds():
    rng = np.random.default_rng(20261019)
    u = lambda n: rng.random((n, 3), dtype=np.float32) - np.float32(0.5)      # noqa: E731

    def shape(n):
        v = rng.standard_normal((n, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        p = (v * np.array([0.5, 0.3, 0.2])).astype(np.float32)
        k = max(1, n // 50)
        p[:k] += (0.3 * rng.standard_normal((k, 3))).astype(np.float32)
        return p

    C = {}
    for n in (1, 5, 21, 63, 64, 65, 255, 256, 257, 700, 2050, 8193):
        C["u%d" % n] = u(n)
    for n in (300, 1000, 3000):
        C["shape%d" % n] = shape(n)
    g = np.arange(8, dtype=np.float32) / np.float32(8)
    C["lattice"] = np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3))
    C["identical300"] = np.repeat(u(1), 300, axis=0)
    C["offset_1e3"] = u(700) + np.float32(1e3)
    C["scale_1e-2"] = u(700) * np.float32(1e-2)
    pl = u(700)
    pl[:, 2] = np.float32(0.25)
    C["plane"] = pl
    C["cluster_far"] = np.concatenate([(0.02 * rng.normal(size=(2000, 3))).astype(np.float32), u(10) + np.float32(50)])
    finite = list(C)
    # added to the issue's generator, after all its draws
    nan = u(700)
    nan[317, 1] = np.nan
    inf = u(700)
    inf[203, 0] = np.inf
    C["nan700"] = nan
    C["inf700"] = inf
    C["empty"] = np.zeros((0, 3), np.float32)
    return C, finite


CLOUDS, FINITE = _clouds()
# the batch: the non-finite clouds and the empty one in the middle, between clouds that must not notice them
ORDER = FINITE[:7] + ["nan700"] + FINITE[7:10] + ["empty"] + FINITE[10:14] + ["inf700"] + FINITE[14:]
assert sorted(ORDER) == sorted(CLOUDS) and ORDER[0] == "u1"


def shape_like(seed, n):
    """A surface like the generator's `shape` clouds, from a stream of its own (test_gpu_fuse_scans.py)."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    p = (v * np.array([0.5, 0.3, 0.2])).astype(np.float32)
    k = max(1, n // 50)
    p[:k] += (0.3 * rng.standard_normal((k, 3))).astype(np.float32)
    return p


def offsets(names):
    off = [0]
    for name in names:
        off.append(off[-1] + CLOUDS[name].shape[0])
    return off


def packed(names):
    return np.ascontiguousarray(np.concatenate([CLOUDS[name] for name in names], axis=0))


_MEANS = {}


def oracle_means(oracle, name, k, mode):
    """oracle.knn_mean_distance of a cloud, computed once per session and never changed (read-only)."""
    key = (name, k, mode)
    if key not in _MEANS:
        P = CLOUDS[name]
        m = oracle.knn_mean_distance(P, k, mode) if P.shape[0] else np.zeros((0,), np.float32)
        m.setflags(write=False)
        _MEANS[key] = m
    return _MEANS[key]


def ordered_sum(v):
    """S(v) of include/genpc_hip.h: 1024 partial sums from +0.0, p[t] adds v[t], v[t + 1024], ... in ascending order; then
    p[t] = p[t] + p[t + w] for w = 512, 256, ..., 1 and t < w; S = p[0]."""
    v = np.asarray(v, np.float64)
    rows = max(1, -(-v.shape[0] // 1024))
    padded = np.zeros(rows * 1024, np.float64)
    padded[:v.shape[0]] = v
    padded = padded.reshape(rows, 1024)
    p = np.zeros(1024, np.float64)
    for r in range(rows):                       # one row at a time: numpy's own sum would pair the rows differently
        p = p + padded[r]
    w = 512
    while w >= 1:
        p = p[:w] + p[w:2 * w]
        w //= 2
    return p[0]


def stats_ref(m, ratio):
    """(mean, std, thr) of a cloud's means in the defined order, every operation a separately rounded float64 operation."""
    m = np.asarray(m, np.float32).astype(np.float64)
    n = m.shape[0]
    if n == 0:
        return np.float64("nan"), np.float64("nan"), np.float64("nan")
    with np.errstate(all="ignore"):
        mean = ordered_sum(m) / np.float64(n)
        d = m - mean
        std = np.sqrt(ordered_sum(d * d) / np.float64(n - 1))
        thr = mean + np.float64(ratio) * std
    return mean, std, thr


def mask_ref(m, ratio):
    with np.errstate(all="ignore"):
        return np.asarray(m, np.float32).astype(np.float64) < stats_ref(m, ratio)[2]


def margin(m, thr):
    """min_i |m_i - thr| / thr where the threshold is positive and finite, else None (nothing lies near a threshold that
    keeps nothing)."""
    if not (np.isfinite(thr) and thr > 0):
        return None
    m = np.asarray(m).astype(np.float64)
    return float(np.min(np.abs(m - thr)) / thr)


def same_bits(a, b):
    """float64 arrays equal bit for bit, any NaN matching any NaN."""
    a, b = np.ascontiguousarray(a, np.float64).ravel(), np.ascontiguousarray(b, np.float64).ravel()
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool(np.array_equal(na, nb)) and bool(np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))
