"""The mesh sampler's definition (include/genpc_hip.h: genpc_mesh_sample) as tests/mesh_sample_ref.py restates it: the random
words are Philox4x32-10, the points lie in their faces, faces of weight zero are never drawn and the faces are drawn in
proportion to their areas.  No GPU; tests/test_gpu_mesh_sample.py holds the kernels to this restatement bit for bit."""
import numpy as np
import pytest

import mesh_sample_ref as R


@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, want):
    got = R.philox4x32_10(counter, key)
    assert tuple(int(g[0]) for g in got) == want


def test_mulhi64_against_python_ints():
    rng = np.random.default_rng(0)
    a = rng.integers(0, 1 << 64, 1000, dtype=np.uint64)
    a[:4] = [0, 1, (1 << 64) - 1, 1 << 63]
    for w in (1, (1 << 63) - 1, (1 << 64) - 1, 0x123456789abcdef, 3 << 38):
        want = [(int(x) * w) >> 64 for x in a]
        assert [int(x) for x in R.mulhi64(a, w)] == want


def test_points_lie_in_their_faces():
    V, F, C = R.grid_mesh(257, seed=1)
    r = R.sample(V, F, 20000, seed=11, colors=C)
    assert r["status"] == 1
    b = r["bary"]
    assert b.dtype == np.float32 and (b >= 0).all()
    # multiples of 2^-24 below 1: their fp32 sums are exact, in either association
    np.testing.assert_array_equal((b[:, 0] + b[:, 1]) + b[:, 2], np.float32(1))
    np.testing.assert_array_equal(b[:, 0] + (b[:, 1] + b[:, 2]), np.float32(1))
    # the point is the barycentric blend of its face's corners (fp64, then the output's fp32 rounding)
    tri = V.astype(np.float64)[F[r["face"]]]
    blend = (tri * b.astype(np.float64)[:, :, None]).sum(axis=1)
    np.testing.assert_allclose(r["points"], blend, rtol=0, atol=2.0 ** -22 * np.abs(V).max())
    assert (r["colors"] >= 0).all() and (r["colors"] <= 1).all()
    # every face of a mesh this small is drawn, none out of range
    assert set(np.unique(r["face"])) == set(range(257))


def test_weights_scale_the_largest_face_to_2_38():
    V, F, _ = R.grid_mesh(100, seed=2)
    for scale in (1.0, 1e-12, 3e11):
        w, cum, bad = R.face_weights((V * scale).astype(np.float32), F)
        assert not bad and (1 << 38) <= int(w.max()) < (1 << 39)
        assert int(cum[-1]) == sum(int(x) for x in w) < 1 << 63


def test_zero_weight_faces_are_never_chosen():
    # face 1 is degenerate (two equal vertices), face 3 has 2^-40 of face 0's area: both weigh 0
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0],
                  [2, 0, 0], [2, 1, 0],
                  [3, 0, 0], [4, 0, 0], [3, 1, 0],
                  [5, 0, 0], [5 + 2.0 ** -20, 0, 0], [5, 2.0 ** -20, 0]], np.float32)
    F = np.array([[0, 1, 2], [3, 3, 4], [5, 6, 7], [8, 9, 10]], np.int32)
    w, cum, bad = R.face_weights(V, F)
    assert not bad and w[1] == 0 and w[3] == 0 and w[0] == w[2] == 1 << 38
    r = R.sample(V, F, 50000, seed=5)
    assert set(np.unique(r["face"])) == {0, 2}
    # nothing can be drawn from a mesh whose faces are all degenerate
    assert R.sample(V, np.array([[3, 3, 4], [0, 0, 0]], np.int32), 10, seed=5)["status"] == -1


def test_bad_faces_are_reported():
    V, F, _ = R.grid_mesh(10, seed=3)
    for bad_index in (len(V), -1):
        G = F.copy()
        G[4, 1] = bad_index
        assert R.sample(V, G, 10, seed=0)["status"] == -1
    U = np.concatenate([V, [[np.nan, 0, 0]]]).astype(np.float32)
    assert R.sample(U, F, 10, seed=0)["status"] == 1              # a vertex no face uses may be anything
    G = F.copy()
    G[7, 2] = len(V)
    assert R.sample(U, G, 10, seed=0)["status"] == -1


def test_prefix_and_seed():
    V, F, _ = R.grid_mesh(50, seed=4)
    a, b = R.sample(V, F, 300, seed=9), R.sample(V, F, 100, seed=9)
    np.testing.assert_array_equal(a["points"][:100], b["points"])
    c = R.sample(V, F, 50, seed=9, first=250)
    np.testing.assert_array_equal(a["points"][250:], c["points"])
    assert not np.array_equal(R.sample(V, F, 100, seed=9 + (1 << 32))["points"], b["points"])      # the key's high word counts


def test_faces_are_drawn_in_proportion_to_area():
    """Two triangles of area 1 : 3, 40 000 samples: the first face's count is binomial(40000, 1/4), sigma = sqrt(7500) =
    86.6; it must lie within 5 sigma of 10 000.  Seed 2024 is fixed (the count it gives is 9 952, checked on the CPU)."""
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 1], [3, 0, 1], [0, 2, 1]], np.float32)      # |e1 x e2| = 2 and 6
    F = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    w, _, _ = R.face_weights(V, F)
    assert int(w[1]) == 3 * int(w[0]) == 3 << 37
    r = R.sample(V, F, 40000, seed=2024)
    n0 = int((r["face"] == 0).sum())
    assert abs(n0 - 10000) <= 5 * np.sqrt(40000 * 0.25 * 0.75), n0
