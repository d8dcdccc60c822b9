"""tests/golden/ref_py_interp.npz guards itself (no GPU): the index table scipy recorded for the reference's
linear_interpolation is the one an exact fp32 search names -- a numpy brute force ordered by the library's 64-bit key
distance bits << 32 | index -- for every one of the 1000 queries, and the recorded float64 outputs follow from the recorded
indices by the reference's arithmetic.  knn_bruteforce / sqdist_fma_exact are also what tests/test_gpu_knn_query.py
compares the HIP library with."""
from fractions import Fraction

import numpy as np
import pytest

F32_INF_BITS = 0x7f800000


def knn_bruteforce(q, t, k):
    """[NQ,3] x [NT,3] float32 -> (dist [NQ,k] float32, idx [NQ,k] int32) in arithmetic mode 0: d = (dx*dx + dy*dy) + dz*dz
    in float32, the k smallest keys d bits << 32 | index among the targets with d < +inf, the rest (+inf, -1)."""
    q, t = np.asarray(q, np.float32), np.asarray(t, np.float32)
    with np.errstate(all="ignore"):
        dx, dy, dz = (t[None, :, a] - q[:, None, a] for a in range(3))
        d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == np.float32
    return select_k(d, k)


def select_k(d, k):
    """float32 distances [NQ,NT] -> the k smallest (distance, index) per row by the 64-bit key."""
    nq, nt = d.shape
    key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(nt, dtype=np.uint64)[None, :]
    with np.errstate(invalid="ignore"):
        key[~(d < np.inf)] = np.uint64(0xffffffffffffffff)
    key = np.sort(key, axis=1)[:, :k]
    if key.shape[1] < k:
        key = np.concatenate([key, np.full((nq, k - key.shape[1]), 0xffffffffffffffff, np.uint64)], axis=1)
    empty = key == np.uint64(0xffffffffffffffff)
    dist = (key >> np.uint64(32)).astype(np.uint32).view(np.float32).copy()
    idx = (key & np.uint64(0xffffffff)).astype(np.int64).astype(np.int32)
    dist[empty] = np.inf
    idx[empty] = -1
    return dist, idx


def round_f32(x):
    """Fraction >= 0 -> the nearest float32 (ties to even), exactly; overflow gives +inf."""
    if x == 0:
        return np.float32(0.0)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    assert Fraction(2) ** e <= x < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    n = x / quantum
    m = n.numerator // n.denominator
    rem = n - m
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and m % 2 == 1):
        m += 1
    v = m * quantum
    if v >= Fraction(2) ** 128:
        return np.float32(np.inf)
    out = np.float32(float(v))          # v has at most 24 significant bits: exact
    assert Fraction(float(out)) == v
    return out


def sqdist_fma_exact(q, t):
    """Arithmetic mode 1 on finite input, with exact rationals: fl(dz dz + fl(dx dx + fl(dy dy))), the differences in
    float32.  [NQ,3] x [NT,3] -> float32 [NQ,NT] (tiny shapes only)."""
    q, t = np.asarray(q, np.float32), np.asarray(t, np.float32)
    out = np.empty((len(q), len(t)), np.float32)
    for i in range(len(q)):
        for j in range(len(t)):
            dx, dy, dz = (Fraction(float(np.float32(t[j, a] - q[i, a]))) for a in range(3))
            s = Fraction(float(round_f32(dy * dy)))
            s = Fraction(float(round_f32(dx * dx + s)))
            out[i, j] = round_f32(dz * dz + s)
    return out


@pytest.fixture(scope="module")
def fx(golden):
    return golden("ref_py_interp.npz")


def test_round_f32_is_numpy_rounding():
    rng = np.random.default_rng(3)
    for v in list(rng.random(200) * 10.0 ** rng.uniform(-44, 38, 200)) + [2.0 ** -149, 2.0 ** -150, 3 * 2.0 ** -150, 1.0 + 2.0 ** -24,
                                                                          1.0 + 3 * 2.0 ** -24, 3.4028235677973366e38, 3.5e38]:
        with np.errstate(over="ignore"):
            assert round_f32(Fraction(float(v))).tobytes() == np.float32(v).tobytes(), v


def test_scipy_index_table_is_the_fp32_key_order(fx):
    """All 1000 queries, all 6 recorded columns: none is left out."""
    dist, idx = knn_bruteforce(fx["interp_queries"].astype(np.float32), fx["interp_points"], 6)
    assert np.array_equal(fx["interp_queries"].astype(np.float32).astype(np.float64), fx["interp_queries"])
    np.testing.assert_array_equal(idx, fx["interp_idx6"])
    np.testing.assert_allclose(np.sqrt(dist.astype(np.float64)), fx["interp_dist6"], rtol=1e-6)
    gap = (fx["interp_dist6"][:, 1:] - fx["interp_dist6"][:, :-1]) / fx["interp_dist6"][:, 1:]
    assert gap.min() > 1e-6


@pytest.mark.parametrize("k", [2, 5])
def test_recorded_outputs_follow_from_recorded_indices(fx, k):
    points, queries, indices = fx["interp_points"].astype(np.float64), fx["interp_queries"], fx["interp_idx6"][:, :k]
    distances = np.sqrt(((points[indices] - queries[:, None, :]) ** 2).sum(axis=2))
    np.testing.assert_allclose(distances, fx["interp_dist6"][:, :k], rtol=1e-14)
    weights = 1 / (distances + 1e-8)
    weights /= weights.sum(axis=1)[:, np.newaxis]
    np.testing.assert_allclose(np.sum(points[indices] * weights[:, :, np.newaxis], axis=1), fx["interp_k%d" % k], rtol=1e-12)


def test_restated_add_points_record(fx):
    assert fx["add_coords"].shape == (512, 3) and fx["add_coords"].dtype == np.float32
    assert fx["add_keep"].shape == (4000,) and fx["add_keep"].dtype == np.bool_ and 0 < fx["add_keep"].sum() < 4000
