"""tests/golden/ref_py_uhd.npz: the reference's own ``UHD`` (metric.py:105-132) on the cases of
tests/golden/make_reference_uhd_vectors.py.  Here (no GPU): the fixture agrees with a plain numpy float64 restatement bit
for bit -- uhd_numpy is also what tests/test_gpu_uhd.py compares the library with where no vector is stored -- and the new
entry point is declared, bound and exported; metric.uhd refuses what it cannot answer."""
import os

import numpy as np
import pytest

from test_abi import header_prototypes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["one", "b3_5x3", "n257_m700", "b2_1000x777", "b2_distinct", "lattice", "identical", "inversion", "scan", "waymo", "split"]


def _load(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def inputs(name, fx=None):
    """(partial [B,N,3], complete [B,M,3]) float32 of a case: stored in ref_py_uhd.npz, or a slice of another fixture."""
    if name == "b3_5x3":
        z = _load("chamfer_seed7_b3_5x3.npz")
        return z["xyz1"], z["xyz2"]
    if name == "b2_1000x777":
        z = _load("chamfer_seed0_b2_1000x777.npz")
        return z["xyz1"], z["xyz2"]
    if name == "identical":
        p = _load("scan01184_fps2048.npz")["partial"]
        return p, p
    if name == "scan":
        z = _load("scans13_fps16384.npz")
        return z["partial"][:1, :4096], z["gt"][:1, :8192]
    if name == "waymo":
        return _load("waymo_car59_4096.npz")["test_partial"][None], _load("waymo_car8_4096.npz")["xyz1"][:1]
    fx = _load("ref_py_uhd.npz") if fx is None else fx
    return fx[name + "_p"], fx[name + "_c"]


def row_minima(p, c, dtype=np.float64, rows=512):
    """min_j s_ij and argmin_j (lowest j) for every query of p [N,3] against c [M,3]; s = ((dx*dx) + (dy*dy)) + (dz*dz),
    d = p - c, in `dtype` with no contraction (numpy has none)."""
    p, c = p.astype(dtype), c.astype(dtype)
    mins, args = [], []
    for i in range(0, len(p), rows):
        d = p[i:i + rows, None, :] - c[None, :, :]
        s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        assert s.dtype == dtype
        args.append(s.argmin(axis=1))
        mins.append(s[np.arange(len(s)), args[-1]])
    return np.concatenate(mins), np.concatenate(args)


def uhd_numpy(P, C):
    """(d2 float64 [B], ij int32 [B,2]) of float32 [B,N,3] / [B,M,3]: max_i min_j s_ij and numpy's argmax / argmin."""
    d2, ij = [], []
    for p, c in zip(P, C):
        m, a = row_minima(p, c)
        i = int(m.argmax())
        d2.append(m[i])
        ij.append((i, int(a[i])))
    return np.array(d2, np.float64), np.array(ij, np.int32)


@pytest.fixture(scope="module")
def fx():
    return _load("ref_py_uhd.npz")


@pytest.mark.parametrize("name", CASES)
def test_fixture_is_the_float64_restatement(fx, name):
    P, C = inputs(name, fx)
    assert P.dtype == np.float32 and C.dtype == np.float32
    d2, ij = uhd_numpy(P, C)
    hd = fx[name + "_hd"]
    assert hd.dtype == np.float64 and hd.shape == (P.shape[0],)
    assert np.array_equal(np.sqrt(d2).view(np.uint64), hd.view(np.uint64)), (np.sqrt(d2), hd)
    assert np.array_equal(ij, fx[name + "_ij"]), (ij, fx[name + "_ij"])


def test_fixture_cases_are_what_they_claim(fx):
    assert fx["b2_distinct_hd"][0] != fx["b2_distinct_hd"][1]
    assert fx["identical_hd"][0] == 0.0 and tuple(fx["identical_ij"][0]) == (0, 0)
    P, C = inputs("split", fx)
    assert P.shape[1] == 65 and C.shape[1] == 513 and fx["split_ij"][0, 1] == 512
    # lattice: several queries attain the maximum and the witness has several nearest targets; the witness is the lowest of each
    P, C = inputs("lattice", fx)
    m, _ = row_minima(P[0], C[0])
    i, j = fx["lattice_ij"][0]
    assert (m == m.max()).sum() > 1 and i == np.flatnonzero(m == m.max())[0]
    d = P[0, i].astype(np.float64) - C[0].astype(np.float64)
    s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert (s == s.min()).sum() > 1 and j == np.flatnonzero(s == s.min())[0]
    # inversion: a float32 search names another query
    P, C = inputs("inversion", fx)
    m32, _ = row_minima(P[0], C[0], np.float32)
    assert int(m32.argmax()) != int(fx["inversion_ij"][0, 0])


def test_genpc_uhd_is_declared_bound_and_exported():
    from genpc_amd import build
    build.build(verbose=False)
    from genpc_amd import _lib
    assert header_prototypes().get("genpc_uhd") == 8
    res, args = _lib.SIGNATURES["genpc_uhd"]
    assert len(args) == 8
    assert getattr(_lib.lib, "genpc_uhd") is not None
    assert _lib.ABI_VERSION >= 19 and _lib.lib.genpc_abi_version() == _lib.ABI_VERSION


def test_uhd_refuses_cpu_tensors():
    import torch
    from genpc_amd import metric
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        metric.uhd(torch.zeros(8, 3), torch.zeros(5, 3))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        metric.uhd(torch.zeros(2, 8, 3), torch.zeros(2, 5, 3), return_witness=True)


def test_uhd_refuses_float64_that_float32_cannot_hold():
    import torch
    from genpc_amd import metric
    bad = torch.full((8, 3), 0.1, dtype=torch.float64)             # 0.1 is not a float32
    ok = torch.full((5, 3), 0.5, dtype=torch.float64)
    with pytest.raises(ValueError, match="float32"):
        metric.uhd(bad, ok)
    with pytest.raises(ValueError, match="float32"):
        metric.uhd(ok, bad)
    with pytest.raises(RuntimeError, match="GPU tensors only"):     # representable: only the device is wrong
        metric.uhd(ok, ok)
    with pytest.raises(TypeError):
        metric.uhd(ok.half(), ok.half())
    with pytest.raises(ValueError):
        metric.uhd(torch.zeros(0, 3), torch.zeros(5, 3))
