"""genpc_uhd (csrc/uhd.hip) and its Python layer (genpc_amd/metric.py: uhd, UHD, evaluate_uhd, cd_emd) on the GPU.

Every kernel check is bit for bit: out_d2 through the C ABI against the numpy float64 restatement
(test_uhd_reference_vectors.uhd_numpy), metric.uhd -- sqrt included -- against what the reference's own UHD returned
(tests/golden/ref_py_uhd.npz), and the witness (i*, j*) against numpy's argmax / argmin.  The cases are the smallest shapes
at which the kernel can go wrong: one pair, sizes that are no multiple of the wave (64), of a workgroup's queries (1024) or
of the target tile (512), several tiles, several batch elements, ties inside and across tiles."""
import numpy as np
import pytest

from test_uhd_reference_vectors import CASES, inputs, row_minima, uhd_numpy

pytestmark = pytest.mark.gpu

TILE = 512          # csrc/uhd.hip: kUhdTile, the targets of one workgroup


@pytest.fixture(scope="module")
def ug():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib, metric
    return dict(torch=torch, _lib=_lib, lib=_lib.lib, metric=metric)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("ref_py_uhd.npz")


def abi_uhd(ug, P, C):
    """genpc_uhd itself on float32 [B,N,3] / [B,M,3] numpy arrays: (d2 float64 [B], ij int32 [B,2])."""
    torch = ug["torch"]
    p, c = torch.from_numpy(np.ascontiguousarray(P)).cuda(), torch.from_numpy(np.ascontiguousarray(C)).cuda()
    d2 = torch.full((p.shape[0],), -7.0, dtype=torch.float64, device="cuda")
    ij = torch.full((p.shape[0], 2), -7, dtype=torch.int32, device="cuda")
    rc = ug["lib"].genpc_uhd(p.shape[0], p.shape[1], p.data_ptr(), c.shape[1], c.data_ptr(), d2.data_ptr(), ij.data_ptr(),
                             ug["_lib"].stream_of(p))
    assert rc == 0, ug["_lib"].last_error()
    return d2.cpu().numpy(), ij.cpu().numpy()


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("name", CASES)
def test_reference_vectors(ug, fx, name):
    torch = ug["torch"]
    P, C = inputs(name, fx)
    want_d2, want_ij = uhd_numpy(P, C)
    d2, ij = abi_uhd(ug, P, C)
    assert same_bits(d2, want_d2), (d2, want_d2)
    assert np.array_equal(ij, want_ij), (ij, want_ij)
    hd, w = ug["metric"].uhd(torch.from_numpy(P).cuda(), torch.from_numpy(C).cuda(), return_witness=True)
    assert hd.dtype == torch.float64 and hd.shape == (P.shape[0],) and w.dtype == torch.int32 and w.shape == (P.shape[0], 2)
    assert same_bits(hd.cpu().numpy(), fx[name + "_hd"]), (hd, fx[name + "_hd"])
    assert np.array_equal(w.cpu().numpy(), fx[name + "_ij"])


def test_batch_elements_have_their_own_answers(ug, fx):
    """a batch stride error would repeat element 0, or read across elements"""
    P, C = inputs("b2_distinct", fx)
    d2, ij = abi_uhd(ug, P, C)
    assert d2[0] != d2[1]
    for b in range(2):
        one_d2, one_ij = abi_uhd(ug, P[b:b + 1], C[b:b + 1])
        assert same_bits(one_d2, d2[b:b + 1]) and np.array_equal(one_ij, ij[b:b + 1])
    swapped, _ = abi_uhd(ug, P[::-1], C[::-1])
    assert same_bits(swapped, d2[::-1])


def test_identical_clouds_tie_across_tiles(ug, fx):
    """every query's minimum is 0, in its own tile: the witness is (0, 0) and nothing else"""
    P, C = inputs("identical", fx)
    assert P.shape[1] == 2048 and C.shape[1] == 4 * TILE
    d2, ij = abi_uhd(ug, P, C)
    assert same_bits(d2, [0.0]) and ij.tolist() == [[0, 0]]


def test_inversion_needs_float64(ug, fx):
    P, C = inputs("inversion", fx)
    m32, _ = row_minima(P[0], C[0], np.float32)
    m64, _ = row_minima(P[0], C[0], np.float64)
    assert int(m32.argmax()) != int(m64.argmax())           # the case still tests something
    _, ij = abi_uhd(ug, P, C)
    assert ij[0, 0] == int(m64.argmax()) and ij[0, 0] != int(m32.argmax())


def test_witness_target_alone_in_the_last_tile(ug, fx):
    P, C = inputs("split", fx)
    assert P.shape[1] == 65 and C.shape[1] == TILE + 1
    d2, ij = abi_uhd(ug, P, C)
    assert ij.tolist() == [[40, TILE]] and same_bits(d2, [0.25])
    # the same target once more in the first tile: a tie between two tiles, and the lower index is the witness
    C2 = C.copy()
    C2[0, 3] = C2[0, TILE]
    want_d2, want_ij = uhd_numpy(P, C2)
    assert want_ij.tolist() == [[40, 3]]
    d2, ij = abi_uhd(ug, P, C2)
    assert ij.tolist() == [[40, 3]] and same_bits(d2, want_d2)


def test_sizes_around_the_tile_and_the_workgroup(ug):
    """N around a workgroup's 1024 queries, M around the 512-target tile, B = 2"""
    rng = np.random.default_rng(1025)
    for n, m in ((1023, 511), (1024, 512), (1025, 513), (64, 1537)):
        P = rng.random((2, n, 3), dtype=np.float32) - np.float32(0.5)
        C = rng.random((2, m, 3), dtype=np.float32) - np.float32(0.5)
        want_d2, want_ij = uhd_numpy(P, C)
        d2, ij = abi_uhd(ug, P, C)
        assert same_bits(d2, want_d2) and np.array_equal(ij, want_ij), (n, m)


def test_non_default_stream(ug, fx):
    torch = ug["torch"]
    P, C = inputs("n257_m700", fx)
    p, c = torch.from_numpy(P).cuda(), torch.from_numpy(C).cuda()
    hd0, w0 = ug["metric"].uhd(p, c, return_witness=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hd1, w1 = ug["metric"].uhd(p, c, return_witness=True)
        hd1, w1 = hd1.cpu(), w1.cpu()                        # the only synchronisation: a copy on the same stream
    assert same_bits(hd1.numpy(), hd0.cpu().numpy()) and same_bits(hd1.numpy(), fx["n257_m700_hd"])
    assert np.array_equal(w1.numpy(), w0.cpu().numpy())


def test_refusals(ug, fx):
    torch = ug["torch"]
    lib, last_error = ug["lib"], ug["_lib"].last_error
    P, C = inputs("n257_m700", fx)
    p, c = torch.from_numpy(P).cuda(), torch.from_numpy(C).cuda()
    d2 = torch.full((1,), -7.0, dtype=torch.float64, device="cuda")
    ij = torch.full((1, 2), -7, dtype=torch.int32, device="cuda")
    args = lambda b, n, m: (b, n, p.data_ptr(), m, c.data_ptr(), d2.data_ptr(), ij.data_ptr(), None)      # noqa: E731
    assert lib.genpc_uhd(*args(1, 0, 700)) == -1 and "genpc_uhd" in last_error()
    assert lib.genpc_uhd(*args(1, 257, 0)) == -1 and "genpc_uhd" in last_error()
    assert lib.genpc_uhd(1, 257, None, 700, c.data_ptr(), d2.data_ptr(), ij.data_ptr(), None) == -1 and "null" in last_error()
    assert lib.genpc_uhd(*args(0, 257, 700)) == 1
    torch.cuda.synchronize()
    assert (d2 == -7.0).all() and (ij == -7).all()
    m = ug["metric"]
    with pytest.raises(ValueError):
        m.uhd(p[0], c[0, :0])
    with pytest.raises(ValueError):
        m.uhd(p, c[0])
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        m.uhd(p.cpu(), c.cpu())


def test_python_forms(ug, fx):
    torch, m = ug["torch"], ug["metric"]
    P, C = inputs("b2_1000x777", fx)
    p, c = torch.from_numpy(P).cuda(), torch.from_numpy(C).cuda()
    hd = m.uhd(p, c)
    one, w = m.uhd(p[1], c[1], return_witness=True)              # unbatched: 0-d and [2]
    assert one.shape == () and w.shape == (2,) and one.item() == hd[1].item() and w.tolist() == fx["b2_1000x777_ij"][1].tolist()
    wide = m.uhd(p.double(), c.double())                          # float32-representable float64 is taken
    assert torch.equal(wide, hd)
    with pytest.raises(ValueError, match="float32"):
        m.uhd(p.double() + 1e-12, c)
    empty = m.uhd(p[:0], c[:0])
    assert empty.shape == (0,) and empty.dtype == torch.float64
    table = m.evaluate_sharded(P, C, metric_fn=m.evaluate_uhd)    # world size 1
    assert table.dtype == torch.float64 and table.shape == (2, 1) and torch.equal(table[:, 0], hd)
    assert same_bits(table[:, 0].cpu().numpy(), fx["b2_1000x777_hd"])


def test_UHD_reads_ply_files(ug, fx, tmp_path, monkeypatch, capsys):
    torch, m = ug["torch"], ug["metric"]
    from genpc_amd.utils.dataUtils import save_ply_xyzrgb
    P, C = inputs("n257_m700", fx)
    pp, cp = str(tmp_path / "partial.ply"), str(tmp_path / "complete.ply")
    save_ply_xyzrgb(P[0], None, pp)
    save_ply_xyzrgb(C[0], None, cp)
    hd = m.UHD(pp, cp)
    assert isinstance(hd, float)
    assert hd == m.uhd(torch.from_numpy(P[0]).cuda(), torch.from_numpy(C[0]).cuda()).item() == float(fx["n257_m700_hd"][0])
    assert m.UHD(pp, pp) == 0.0
    monkeypatch.setattr("sys.argv", ["metric", "--uhd", pp, cp])
    m.main()
    assert capsys.readouterr().out.strip() == "UHD: %.2f" % (hd * 100)
    bad = str(tmp_path / "double.ply")                            # a PLY of genuine doubles is refused, not rounded
    save_ply_xyzrgb(P[0].astype(np.float64) + 1e-12, None, bad)
    with pytest.raises(ValueError, match="float32"):
        m.UHD(bad, cp)


def test_cd_emd_is_the_composition(ug, golden, tmp_path):
    torch, m = ug["torch"], ug["metric"]
    from genpc_amd.fps import fps_subsample
    from genpc_amd.utils.dataUtils import save_ply_xyzrgb
    g = golden("scans13_fps16384.npz")
    a, b = g["gt"][0], g["partial"][0]
    pa, pb = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    save_ply_xyzrgb(a, None, pa)
    save_ply_xyzrgb(b, None, pb)
    cd, emd = m.cd_emd(pa, pb)
    # the same clouds in the order the (deterministic) subsampling leaves them: gen = cloud 2, gt = cloud 1
    sa = fps_subsample(torch.from_numpy(a).cuda()[None], 16384)
    sb = fps_subsample(torch.from_numpy(b).cuda()[None], 16384)
    row = m.evaluate_scans(sb, sa)[0]
    # the per-point values are the same; the two fp32 means of 16384 values are reduced by different calls, each within
    # log2(16384) * 2^-24 = 8.3e-7 relative of the exact mean for a tree sum: 2e-6 between them
    assert abs(cd.item() - row[0].item()) <= 2e-6 * row[0].item()
    assert abs(emd.item() - row[2].item()) <= 2e-6 * row[2].item()
