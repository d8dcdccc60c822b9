"""genpc_uhd_ragged (csrc/uhd_ragged.hip) and its Python layer (genpc_amd/metric.py: uhd_ragged, score_uhd_folders,
--uhd-dirs) on the GPU.

Every check is bit for bit: out_d2 against the numpy float64 restatement (test_uhd_reference_vectors.uhd_numpy), its sqrt
against what the reference's own UHD returned (tests/golden/ref_py_uhd.npz), the witness against numpy's argmax / argmin,
and each pair against genpc_uhd on that pair alone.  Every ABI call pre-fills out_d2 / out_ij with a sentinel and allocates
one element more than c: the extra one must come back untouched.  The shapes are the smallest at which the kernels can go
wrong: sizes that are no multiple of the wave (64), of a workgroup's 1024 queries or of the targets one workgroup covers,
pair boundaries inside a workgroup's query range, a single pair, the full table of 384."""
import ctypes

import numpy as np
import pytest

from test_uhd_reference_vectors import CASES, inputs, row_minima, uhd_numpy

pytestmark = pytest.mark.gpu

TILE = 512                # csrc/uhd.h: kUhdTile
WG_TARGETS = 1 * TILE     # csrc/uhd_ragged.hip: the targets one workgroup of uhd_ragged_pairs_kernel covers (one tile, blockIdx.y)
WG_QUERIES = 1024         # ... and the queries it owns (kUhdRaggedShift = 10)
MAX_PAIRS = 384
SENT = -7


@pytest.fixture(scope="module")
def ug():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib, metric
    return dict(torch=torch, _lib=_lib, lib=_lib.lib, metric=metric)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("ref_py_uhd.npz")


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def offsets(clouds):
    return [0] + [int(v) for v in np.cumsum([len(c) for c in clouds])]


def raw_call(ug, c, noff, moff, p, t, stream=None, slots=None):
    """genpc_uhd_ragged as it is: (rc, d2 [slots] float64, ij [slots,2] int32) after a synchronise, sentinel where unwritten.
    noff / moff: Python ints or None; p / t: device tensors or None."""
    torch = ug["torch"]
    slots = max(c, 0) + 1 if slots is None else slots
    d2 = torch.full((slots,), float(SENT), dtype=torch.float64, device="cuda")
    ij = torch.full((slots, 2), SENT, dtype=torch.int32, device="cuda")
    na = None if noff is None else (ctypes.c_int * len(noff))(*noff)
    ma = None if moff is None else (ctypes.c_int * len(moff))(*moff)
    cast = lambda a: None if a is None else ctypes.cast(a, ctypes.c_void_p)      # noqa: E731
    rc = ug["lib"].genpc_uhd_ragged(c, cast(na), None if p is None else p.data_ptr(), cast(ma), None if t is None else t.data_ptr(),
                                    d2.data_ptr(), ij.data_ptr(), stream)
    torch.cuda.synchronize()
    return rc, d2.cpu().numpy(), ij.cpu().numpy()


def abi_ragged(ug, pairs):
    """genpc_uhd_ragged on a list of (queries [N_j,3], targets [M_j,3]) float32 numpy arrays: (d2 float64 [c], ij int32 [c,2])."""
    torch = ug["torch"]
    c = len(pairs)
    p = torch.from_numpy(np.ascontiguousarray(np.concatenate([a for a, _ in pairs]))).cuda()
    t = torch.from_numpy(np.ascontiguousarray(np.concatenate([b for _, b in pairs]))).cuda()
    rc, d2, ij = raw_call(ug, c, offsets([a for a, _ in pairs]), offsets([b for _, b in pairs]), p, t, ug["_lib"].stream_of(p))
    assert rc == 0, ug["_lib"].last_error()
    assert d2[c] == SENT and (ij[c] == SENT).all(), "the element behind the last pair was written"
    return d2[:c], ij[:c]


def abi_uhd_one(ug, a, b):
    """genpc_uhd with B = 1 on one pair: (d2 float64, ij int32 [2])."""
    torch = ug["torch"]
    p, t = torch.from_numpy(np.ascontiguousarray(a)).cuda(), torch.from_numpy(np.ascontiguousarray(b)).cuda()
    d2 = torch.full((1,), float(SENT), dtype=torch.float64, device="cuda")
    ij = torch.full((1, 2), SENT, dtype=torch.int32, device="cuda")
    rc = ug["lib"].genpc_uhd(1, len(a), p.data_ptr(), len(b), t.data_ptr(), d2.data_ptr(), ij.data_ptr(), ug["_lib"].stream_of(p))
    assert rc == 0, ug["_lib"].last_error()
    return d2.cpu().numpy()[0], ij.cpu().numpy()[0]


def numpy_pairs(pairs):
    d2, ij = zip(*(uhd_numpy(a[None], b[None]) for a, b in pairs))
    return np.concatenate(d2), np.concatenate(ij)


@pytest.fixture(scope="module")
def ref(fx):
    """The 15 pairs of the 11 recorded cases with the reference's own hd and witness."""
    pairs, hd, ij = [], [], []
    for name in CASES:
        P, C = inputs(name, fx)
        for b in range(P.shape[0]):
            pairs.append((np.ascontiguousarray(P[b]), np.ascontiguousarray(C[b])))
            hd.append(fx[name + "_hd"][b])
            ij.append(fx[name + "_ij"][b])
    assert len(pairs) == 15
    sizes = [(len(a), len(b)) for a, b in pairs]
    assert (1, 1) in sizes and (4096, 8192) in sizes
    return dict(pairs=pairs, hd=np.array(hd, np.float64), ij=np.array(ij, np.int32))


@pytest.fixture(scope="module")
def batch(ug, ref):
    """the 15 pairs as ONE ragged call through the C ABI, computed once"""
    return abi_ragged(ug, ref["pairs"])


def test_reference_values_through_the_abi(ref, batch):
    d2, ij = batch
    assert same_bits(np.sqrt(d2), ref["hd"]), (np.sqrt(d2), ref["hd"])
    assert np.array_equal(ij, ref["ij"]), (ij, ref["ij"])
    a, b = ref["pairs"][11]                                               # inversion: a float32 search names another query
    m32, _ = row_minima(a, b, np.float32)
    assert ij[11, 0] != int(m32.argmax())


def test_reference_values_through_metric_list_and_packed(ug, ref):
    torch, m = ug["torch"], ug["metric"]
    P = [torch.from_numpy(a).cuda() for a, _ in ref["pairs"]]
    C = [torch.from_numpy(b).cuda() for _, b in ref["pairs"]]
    from genpc_amd.loss_functions.Chamfer3D.dist_chamfer_ragged import pack_clouds
    packed_p, packed_c = pack_clouds(P), pack_clouds(C)
    for args in ((P, C), (packed_p, packed_c), (P, (packed_c[0], torch.tensor(packed_c[1])))):
        hd, w = m.uhd_ragged(*args, return_witness=True)
        assert hd.dtype == torch.float64 and hd.shape == (15,) and hd.is_cuda and w.dtype == torch.int32 and w.shape == (15, 2)
        assert same_bits(hd.cpu().numpy(), ref["hd"]), (hd, ref["hd"])
        assert np.array_equal(w.cpu().numpy(), ref["ij"])
    assert torch.equal(m.uhd_ragged(P, C), hd)
    wide = m.uhd_ragged([p.double() for p in P[:4]], C[:4])              # float32-representable float64 is taken
    assert torch.equal(wide, hd[:4])
    with pytest.raises(ValueError, match="float32"):
        m.uhd_ragged([P[0].double() + 1e-12], C[:1])
    empty, w = m.uhd_ragged([], [], return_witness=True)
    assert empty.shape == (0,) and empty.dtype == torch.float64 and w.shape == (0, 2) and w.dtype == torch.int32
    with pytest.raises(ValueError, match="pair 1 has an empty cloud"):
        m.uhd_ragged([P[0], P[1][:0]], C[:2])
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        m.uhd_ragged([p.cpu() for p in P[:2]], [c.cpu() for c in C[:2]])


def test_reversed_and_shuffled_order(ug, ref, batch):
    d2, ij = batch
    perm = np.random.default_rng(15).permutation(15)
    assert not np.array_equal(perm, np.arange(15))
    for order in (np.arange(15)[::-1], perm):
        got_d2, got_ij = abi_ragged(ug, [ref["pairs"][k] for k in order])
        assert same_bits(got_d2, d2[order]) and np.array_equal(got_ij, ij[order]), order


def test_each_pair_alone_and_through_genpc_uhd(ug, ref, batch):
    d2, ij = batch
    for k, (a, b) in enumerate(ref["pairs"]):
        one_d2, one_ij = abi_ragged(ug, [(a, b)])                         # c = 1
        assert same_bits(one_d2, d2[k:k + 1]) and np.array_equal(one_ij, ij[k:k + 1]), k
        rect_d2, rect_ij = abi_uhd_one(ug, a, b)
        assert same_bits(rect_d2, d2[k]) and np.array_equal(rect_ij, ij[k]), k


def test_sizes_around_the_workgroup(ug):
    """query counts around the wave and a workgroup's 1024 queries, target counts around the tile and around what one
    workgroup covers, packed so that the pair boundaries fall inside a workgroup's query range"""
    shapes = [(1, 513), (63, 1), (64, 511), (65, 512), (1023, 1537), (1024, WG_TARGETS - 1), (1025, WG_TARGETS), (2049, WG_TARGETS + 1),
              (2048, 700), (1000, 3 * WG_TARGETS + 1)]
    assert {n for n, _ in shapes} >= {1, 63, 64, 65, 1023, 1024, 1025, 2049}
    assert {m for _, m in shapes} >= {1, 511, 512, 513, 1537, WG_TARGETS - 1, WG_TARGETS, WG_TARGETS + 1}
    starts = offsets([np.empty((n, 3)) for n, _ in shapes])[:-1]
    assert all(s % WG_QUERIES for s in starts[1:])                        # no boundary is aligned: each lies inside a 1024-range
    at = dict(zip([n for n, _ in shapes], starts))
    assert at[1024] % WG_QUERIES and at[2048] % WG_QUERIES                # multiples of 1024 at unaligned offsets
    rng = np.random.default_rng(2049)
    pairs = [(rng.random((n, 3), dtype=np.float32) - np.float32(0.5), rng.random((m, 3), dtype=np.float32) - np.float32(0.5))
             for n, m in shapes]
    want_d2, want_ij = numpy_pairs(pairs)
    d2, ij = abi_ragged(ug, pairs)
    assert same_bits(d2, want_d2), (d2, want_d2)
    assert np.array_equal(ij, want_ij), (ij, want_ij)


def test_ties_take_the_lowest_index_on_both_sides(ug, fx):
    P, C = inputs("split", fx)
    assert P.shape[1] == 65 and C.shape[1] == TILE + 1
    # the witness target once more in the first tile: a tie between two workgroups' targets, the lower index is the witness
    C2 = C.copy()
    C2[0, 3] = C2[0, TILE]
    assert uhd_numpy(P, C2)[1].tolist() == [[40, 3]]
    rng = np.random.default_rng(7)
    same = rng.random((1500, 3), dtype=np.float32)                        # two identical clouds: every minimum is 0
    pairs = [(P[0], C[0]), (same, same), (P[0], C2[0])]
    want_d2, want_ij = numpy_pairs(pairs)
    assert want_ij.tolist() == [[40, TILE], [0, 0], [40, 3]] and want_d2.tolist() == [0.25, 0.0, 0.25]
    d2, ij = abi_ragged(ug, pairs)
    assert same_bits(d2, want_d2) and np.array_equal(ij, want_ij), (d2, ij)


def test_384_pairs_and_one_more(ug):
    torch = ug["torch"]
    rng = np.random.default_rng(384)
    pairs = [(rng.random((int(n), 3), dtype=np.float32), rng.random((int(m), 3), dtype=np.float32))
             for n, m in rng.integers(1, 6, (MAX_PAIRS + 1, 2))]
    want_d2, want_ij = numpy_pairs(pairs)
    d2, ij = abi_ragged(ug, pairs[:MAX_PAIRS])
    assert same_bits(d2, want_d2[:MAX_PAIRS]) and np.array_equal(ij, want_ij[:MAX_PAIRS])
    # 385: the ABI refuses, metric.uhd_ragged splits
    p = torch.from_numpy(np.concatenate([a for a, _ in pairs])).cuda()
    t = torch.from_numpy(np.concatenate([b for _, b in pairs])).cuda()
    rc, d2, ij = raw_call(ug, MAX_PAIRS + 1, offsets([a for a, _ in pairs]), offsets([b for _, b in pairs]), p, t)
    assert rc == -1 and "384" in ug["_lib"].last_error() and (d2 == SENT).all() and (ij == SENT).all()
    hd, w = ug["metric"].uhd_ragged([torch.from_numpy(a).cuda() for a, _ in pairs], [torch.from_numpy(b).cuda() for _, b in pairs],
                                    return_witness=True)
    assert same_bits(hd.cpu().numpy(), np.sqrt(want_d2)) and np.array_equal(w.cpu().numpy(), want_ij)


def test_non_finite_input_stays_in_its_pair(ug):
    rng = np.random.default_rng(99)
    mk = lambda n, m: (rng.random((n, 3), dtype=np.float32), rng.random((m, 3), dtype=np.float32))      # noqa: E731
    pairs = [mk(300, 700), mk(70, 600), mk(1100, 90)]
    clean_d2, clean_ij = numpy_pairs([pairs[0], pairs[2]])
    pairs[1][0][5, 2] = np.nan                                            # a NaN query ...
    pairs[1][1][520, 1] = np.inf                                          # ... and a +inf target coordinate, in the second tile
    d2, ij = abi_ragged(ug, pairs)
    assert same_bits(d2[[0, 2]], clean_d2) and np.array_equal(ij[[0, 2]], clean_ij)
    rect_d2, rect_ij = abi_uhd_one(ug, *pairs[1])
    assert same_bits(d2[1], rect_d2) and ij[1, 0] == rect_ij[0]
    assert d2[1] == np.inf and ij[1, 0] == 5                              # query 5 has no finite pair; never NaN, i* valid
    # j*: the lowest target of the pair with s == d2 for query i*, -1 if none has
    with np.errstate(invalid="ignore"):
        d = pairs[1][0][ij[1, 0]].astype(np.float64) - pairs[1][1].astype(np.float64)
        s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    hits = np.flatnonzero(s == d2[1])
    assert ij[1, 1] == (hits[0] if len(hits) else -1) == -1
    # an infinite minimum that a target attains: the query at +inf is at s = +inf from every target, the lowest is the witness
    pairs[1][0][5] = (np.inf, 0.0, 0.0)
    pairs[1][1][520, 1] = 0.5
    d2, ij = abi_ragged(ug, pairs)
    assert same_bits(d2[[0, 2]], clean_d2) and np.array_equal(ij[[0, 2]], clean_ij)
    assert d2[1] == np.inf and ij[1].tolist() == [5, 0]


def test_refusals_write_nothing(ug, fx):
    torch, last_error = ug["torch"], ug["_lib"].last_error
    P, C = inputs("n257_m700", fx)
    p, t = torch.from_numpy(P[0]).cuda(), torch.from_numpy(C[0]).cuda()

    def refused(c, noff, moff, qp=p, tp=t, what="genpc_uhd_ragged"):
        rc, d2, ij = raw_call(ug, c, noff, moff, qp, tp, slots=3)
        assert rc == -1 and what in last_error(), (rc, last_error())
        assert (d2 == SENT).all() and (ij == SENT).all()
    refused(2, [0, 257, 257], [0, 300, 700], what="pair 1 has no queries")
    refused(2, [0, 100, 257], [0, 700, 700], what="no targets")
    refused(2, [0, 0, 257], [0, 0, 700], what="pair 0 has no queries")           # empty on both sides
    refused(1, [0, 0], [0, 0])
    refused(2, [0, 200, 100], [0, 300, 700], what="ascend")
    refused(2, [0, 100, 257], [0, 700, 300], what="ascend")
    refused(2, [1, 100, 257], [0, 300, 700], what="start at 0")
    refused(2, [0, 100, 257], [1, 300, 700], what="start at 0")
    refused(2, [0, 100, 257], [0, 300, 700], qp=None, what="null")
    refused(2, [0, 100, 257], [0, 300, 700], tp=None, what="null")
    refused(2, None, [0, 300, 700], what="null")
    refused(-1, [0, 257], [0, 700], what="negative")
    rc, d2, ij = raw_call(ug, 2, [0, 100, 257], [0, 300, 700], p, t, slots=3)     # (the arguments were good ones)
    assert rc == 0 and (d2[:2] != SENT).all() and d2[2] == SENT
    lib = ug["lib"]
    out = torch.full((1,), float(SENT), dtype=torch.float64, device="cuda")
    assert lib.genpc_uhd_ragged(2, ctypes.cast((ctypes.c_int * 3)(0, 100, 257), ctypes.c_void_p), p.data_ptr(),
                                ctypes.cast((ctypes.c_int * 3)(0, 300, 700), ctypes.c_void_p), t.data_ptr(), None, out.data_ptr(), None) == -1
    rc, d2, ij = raw_call(ug, 0, [0], [0], p, t)
    assert rc == 1 and (d2 == SENT).all() and (ij == SENT).all()
    rc, d2, ij = raw_call(ug, 0, None, None, None, None)
    assert rc == 1


def test_non_default_stream(ug, ref):
    torch, m = ug["torch"], ug["metric"]
    P = [torch.from_numpy(a).cuda() for a, _ in ref["pairs"][:6]]
    C = [torch.from_numpy(b).cuda() for _, b in ref["pairs"][:6]]
    hd0, w0 = m.uhd_ragged(P, C, return_witness=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hd1, w1 = m.uhd_ragged(P, C, return_witness=True)
        hd1, w1 = hd1.cpu(), w1.cpu()                        # the only synchronisation: a copy on the same stream
    assert same_bits(hd1.numpy(), hd0.cpu().numpy()) and same_bits(hd1.numpy(), ref["hd"][:6])
    assert np.array_equal(w1.numpy(), w0.cpu().numpy())


def test_folders_and_the_command_line(ug, ref, tmp_path, monkeypatch, capsys):
    m = ug["metric"]
    from genpc_amd.utils.dataUtils import save_ply_xyzrgb
    pdir, cdir = tmp_path / "partial", tmp_path / "complete"
    pdir.mkdir()
    cdir.mkdir()
    picks = {"b.ply": ref["pairs"][4], "a.ply": ref["pairs"][5], "c.ply": ref["pairs"][1]}       # 257 x 700, 1000 x 777, 5 x 3
    assert len({(len(a), len(b)) for a, b in picks.values()}) == 3
    for name, (a, b) in picks.items():
        save_ply_xyzrgb(a, None, str(pdir / name))
        save_ply_xyzrgb(b, None, str(cdir / name))
    save_ply_xyzrgb(ref["pairs"][0][0], None, str(pdir / "lonely_partial.ply"))
    save_ply_xyzrgb(ref["pairs"][0][1], None, str(cdir / "lonely_complete.ply"))
    names, hds, only_p, only_c = m.score_uhd_folders(str(pdir), str(cdir))
    assert names == ["a.ply", "b.ply", "c.ply"] and only_p == ["lonely_partial.ply"] and only_c == ["lonely_complete.ply"]
    assert isinstance(hds, np.ndarray) and hds.dtype == np.float64 and hds.shape == (3,)
    singles = [m.UHD(str(pdir / n), str(cdir / n)) for n in names]
    assert [float(v) for v in hds] == singles
    assert singles == [float(ref["hd"][5]), float(ref["hd"][4]), float(ref["hd"][1])]
    monkeypatch.setattr("sys.argv", ["metric", "--uhd-dirs", str(pdir), str(cdir)])
    m.main()
    total = 0
    for v in singles:
        total += v
    want = ["%s : %.2f" % (n, v * 100) for n, v in zip(names, singles)]
    want += ["lonely_partial.ply : no counterpart in COMPLETE_DIR", "lonely_complete.ply : no counterpart in PARTIAL_DIR"]
    want += ["UHD: %.2f" % (total / 3 * 100)]
    assert capsys.readouterr().out.splitlines() == want
