"""genpc_knn_mean_distance (csrc/knn.hip) on the GPU: reg_xyz.knn_mean_distance against oracle.knn_mean_distance (an
exhaustive loop on the CPU), bit for bit and NaN for NaN, in both arithmetic modes, on the smallest clouds at which a search
through a grid can go wrong: the sizes around 256, fewer points than k, exact ties at the k-th place, zero extent, coordinates
far from the origin and at other scales, inactive axes, empty cells between a cluster and far points, the size at which the
grid's build changes its number of pieces, repeated points, a NaN and an infinite coordinate."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _clouds():
    rng = np.random.default_rng(20261018)
    u = lambda n: rng.random((n, 3), dtype=np.float32) - np.float32(0.5)      # noqa: E731
    c = {}
    c["n256"] = u(256)
    c["n257"] = u(257)
    c["n1"] = u(1)
    c["n5"] = u(5)
    g = np.arange(8, dtype=np.float32) / np.float32(8)
    c["lattice"] = np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3))
    c["identical300"] = np.repeat(u(1), 300, axis=0)
    c["offset_1e3"] = u(700) + np.float32(1e3)
    c["scale_1e-2"] = u(700) * np.float32(1e-2)
    c["scale_1e2"] = u(700) * np.float32(1e2)
    plane = u(700)
    plane[:, 2] = np.float32(0.25)
    c["plane"] = plane
    line = u(700)
    line[:, 1] = np.float32(-0.125)
    line[:, 2] = np.float32(3.0)
    c["line"] = line
    c["cluster_far"] = np.concatenate([(0.02 * rng.normal(size=(2000, 3))).astype(np.float32), u(10) + np.float32(50)])
    c["n8193"] = u(8193)
    c["tripled"] = np.ascontiguousarray(np.tile(u(233), (3, 1))[rng.permutation(699)])
    nan = u(700)
    nan[317, 1] = np.nan
    c["nan"] = nan
    inf = u(700)
    inf[203, 0] = np.inf
    c["inf"] = inf
    return c


CLOUDS = _clouds()
CASES = [(name, k) for name in CLOUDS for k in (8, 20)] + [(name, k) for name in ("lattice", "n8193") for k in (16, 32)]


@pytest.fixture(scope="module")
def km():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib, reg_xyz
    return dict(torch=torch, lib=_lib.lib, R=reg_xyz)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,k", CASES)
def test_knn_mean_equals_oracle(km, oracle, name, k, mode):
    P = CLOUDS[name]
    prev = km["lib"].genpc_set_arith(mode)
    try:
        m = km["R"].knn_mean_distance(km["torch"].from_numpy(P).cuda(), k).cpu().numpy()
    finally:
        km["lib"].genpc_set_arith(prev)
    assert m.shape == (P.shape[0],) and m.dtype == np.float32
    np.testing.assert_array_equal(m, oracle.knn_mean_distance(P, k, mode))
