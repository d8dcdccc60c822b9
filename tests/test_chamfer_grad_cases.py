"""tests/chamfer_grad_cases.py builds what it says (no GPU): the constants its model of chamfer_grad_dir_kernel restates are
the code's, every named case reaches the paths tests/test_gpu_chamfer_backward.py runs it for, the lattice flavour is exact
in fp32 in any order, and `reference` agrees with the pinned sequential oracle."""
import os
import re

import numpy as np
import pytest

import chamfer_grad_cases as C

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "genpc_amd", "csrc")


def _source(path):
    return open(os.path.join(CSRC, path)).read()


def _constant(path, name):
    m = re.search(r"\b%s\s*=\s*(\d+)\s*;" % name, _source(path))
    assert m, (path, name)
    return int(m.group(1))


@pytest.fixture(scope="module")
def cen():
    return {name: C.census(C.Case(name, None, *C.SHAPES[name], None, None, None, None, *C.indices(name), None, None))
            for name in C.CASES}


def test_what_the_kernel_constants_are():
    src = _source("chamfer.hip")
    assert _constant("chamfer.hip", "kGradTile") == C.GRAD_TILE
    assert _constant("chamfer.hip", "kGradList") == C.GRAD_LIST
    assert _constant("chamfer.hip", "kGradBlock") == C.GRAD_BLOCK
    assert _constant("common.h", "kWave") == C.WAVE
    m = re.search(r"\(long long\)b \* \(\(long long\)n \+ m\) >= (\d+)\)", src)
    assert m and int(m.group(1)) == C.THRESHOLD
    # what the model restates of the kernel's control flow: eight entries per thread and trip, the three ways, the two decodes
    assert "q0 += %d * kGradBlock" % C.SLOTS in src and "int kk[%d]" % C.SLOTS in src
    assert "if (total == 0) continue;" in src and "if (total <= kGradList)" in src
    assert "if ((b & 7) == 0) { const int xcd = lin & 7, k = lin >> 3; e = 8 * (k / tiles) + xcd; tile = k % tiles; }" in src
    assert "else { e = lin / tiles; tile = lin % tiles; }" in src
    assert "const int rows = min(kGradTile, nt - t0);" in src


def test_sizes_sit_where_the_table_says():
    pts = {name: b * (n + m) for name, (b, n, m) in C.SHAPES.items()}
    assert pts["threshold"] == C.THRESHOLD and pts["threshold_minus_1"] == C.THRESHOLD - 1
    for name in C.TILE_CASES:          # just over the threshold: every GPU test stays small
        assert C.THRESHOLD <= pts[name] <= C.THRESHOLD + C.THRESHOLD // 20, name
    for name in C.SMALL:
        assert pts[name] < 4096, name
    i1, i2 = C.indices("threshold")
    j1, j2 = C.indices("threshold_minus_1")
    assert j1.max() < C.SHAPES["threshold_minus_1"][2] and j2.shape[1] == i2.shape[1] - 1
    for name, (b, n, m) in C.SHAPES.items():
        i1, i2 = C.indices(name)
        assert i1.shape == (b, n) and i2.shape == (b, m) and i1.dtype == np.int32 and i2.dtype == np.int32
        assert 0 <= i1.min() and i1.max() < m and 0 <= i2.min() and i2.max() < n, name


def test_each_case_reaches_what_its_row_says(cen):
    c = cen["threshold"]
    assert c["kernel"] == "tile" and c["decode"] == "plain"
    assert [d["tiles"] for d in c["dirs"]] == [28, 37]
    for d in c["dirs"]:
        assert d["tiles_hit"] == list(range(d["tiles"])) and d["short_last_tile_past_first_hit"]
        assert d["list_slots"] == set(range(8)) and 8 in d["list_slot_counts"]
    assert cen["threshold_minus_1"]["kernel"] == "atomic" and cen["threshold_minus_1"]["points"] == C.THRESHOLD - 1

    c = cen["batch3"]
    assert c["kernel"] == "tile" and c["decode"] == "plain" and c["e_max"] == 2
    c = cen["batch8"]
    assert c["kernel"] == "tile" and c["decode"] == "xcd" and c["k_over_tiles_max"] == 0
    assert all(d["tiles"] > 1 and d["tiles_hit"] == list(range(d["tiles"])) for d in c["dirs"])
    assert c["dirs"][0]["list_trips"] > 0 and c["dirs"][0]["inplace_trips"] > 0           # mixed in one launch
    c = cen["batch16"]
    assert c["kernel"] == "tile" and c["decode"] == "xcd" and c["k_over_tiles_max"] == 1

    c = cen["list_boundary"]
    d0, d1 = c["dirs"]
    assert c["kernel"] == "tile" and d0["tiles"] == 2 and d0["tiles_hit"] == [0, 1] and d0["skip_trips"] == 0
    # tile 0 has every total of 120 ... 135: lists up to 128, in place from 129; tile 1 has the rest of the 512, in place
    assert d0["totals"] == set(range(120, 136)) | set(512 - t for t in range(120, 136))
    assert d0["list_trips"] == sum(1 for t in range(31) for w in range(16) if 120 + (w + t) % 16 <= C.GRAD_LIST)
    assert d0["list_trips"] + d0["inplace_trips"] == 2 * 31 * 16 and d0["list_slots"] == {0, 1}
    assert d0["tiles_per_wave_trip"] == 2 and d1["tiles_per_wave_trip"] > 2

    c = cen["few_queries"]
    d0 = c["dirs"][0]
    assert c["kernel"] == "tile" and d0["queries"] == 300 < C.GRAD_BLOCK and d0["trips"] == 1
    assert d0["skip_trips"] > 0 and d0["list_trips"] > 0 and d0["list_slots"] == {0}
    c = cen["single_query"]
    d0, d1 = c["dirs"]
    assert c["kernel"] == "tile" and d0["queries"] == 1 and d0["list_trips"] == 1 and d0["totals"] == {0, 1}
    assert d1["tiles"] == 1 and d1["rows_last"] == 1 and d1["one_row_tile_hit"] and d1["max_row_terms"] == 262143
    assert d1["totals"] == {511, 512} and d1["list_trips"] == 0

    c = cen["one_row_tile"]
    d0, d1 = c["dirs"]
    assert c["kernel"] == "tile" and d0["tiles"] == 64 and d0["rows_last"] == 1 and d0["one_row_tile_hit"]
    assert d0["max_row_terms"] >= 200 and d1["tiles"] == 1 and d1["rows_last"] == 4095 and d1["short_last_tile_hit"]
    c = cen["crowded_last_row"]
    d0 = c["dirs"][0]
    assert c["kernel"] == "tile" and d0["tiles"] == 2 and d0["rows_last"] == 1 and d0["tiles_hit"] == [1]
    assert d0["max_row_terms"] == 258048 and d0["one_row_tile_hit"] and d0["totals"] == {0, 256, 512}
    assert d0["skip_trips"] == d0["inplace_trips"] > 0 and d0["list_trips"] == 0

    for name in C.SMALL:
        assert cen[name]["kernel"] == "atomic", name
    assert cen["small_5_257_255"]["directions_meet_in_a_wave"] and cen["small_2_1_700"]["directions_meet_in_a_wave"]
    for name, cloud in (("small_2_1_700", 1), ("small_2_700_1", 0)):          # all of one cloud on one row
        assert not C.indices(name)[cloud].any()


def test_all_cases_together_reach_every_path(cen):
    dirs = [d for c in cen.values() for d in c["dirs"]]
    assert {c["decode"] for c in cen.values()} == {"plain", "xcd", None}
    assert {c["kernel"] for c in cen.values()} == {"tile", "atomic"}
    assert set().union(*(d["list_slots"] for d in dirs)) == set(range(8))
    assert any(8 in d["list_slot_counts"] for d in dirs)
    # (the last slot feeds a list only where an index array of 8 kGradBlock entries or more is spread over enough tiles:
    # these are the cases in which a list that drops or misplaces slot 7 shows)
    assert {n for n, c in cen.items() if any(7 in d["list_slots"] for d in c["dirs"])} == {"threshold", "batch3", "batch8", "list_boundary"}
    assert {127, 128, 129} <= set().union(*(d["totals"] for d in dirs))
    assert any(d["inplace_trips"] for d in dirs) and any(d["skip_trips"] for d in dirs) and any(d["list_trips"] for d in dirs)
    assert any(d["hits_past_first_tile"] for d in dirs)
    assert any(d["short_last_tile_past_first_hit"] for d in dirs)
    assert any(d["one_row_tile_hit"] for d in dirs)
    assert any(d["tiles_per_wave_trip"] > 1 for d in dirs)          # one block per entry is put at risk
    assert any(c["points"] == C.THRESHOLD for c in cen.values()) and any(c["points"] == C.THRESHOLD - 1 for c in cen.values())
    assert any(c["decode"] == "plain" and c["e_max"] > 0 for c in cen.values())
    assert any(c["decode"] == "xcd" and c["k_over_tiles_max"] > 0 for c in cen.values())


def test_what_the_old_large_call_test_does_not_reach():
    """tests/test_gpu_chamfer.py::test_backward_large_call_forms, for contrast: why the cases above exist.  (Its direction 0
    has ONE tile, of 3000 rows: hits are tested against rows < kGradTile there, at t0 = 0 only.)"""
    c = C.census(C.old_large_call_inputs())
    d0, d1 = c["dirs"]
    assert c["kernel"] == "tile" and c["decode"] == "xcd"            # the plain decode is never taken
    assert d0["tiles"] == 1 and d1["tiles"] == 3 and d1["rows_last"] == 904
    assert d1["tiles_hit"] == [0]                                      # the 904-row tile flushes zeros
    for d in (d0, d1):
        assert not d["hits_past_first_tile"] and not d["short_last_tile_past_first_hit"] and not d["one_row_tile_hit"]
        assert d["tiles_per_wave_trip"] == 1                           # no index array's hits are spread over tiles
        assert d["list_slots"] <= {0, 1} and max(d["list_slot_counts"]) <= 2
        assert not {127, 129} & d["totals"]
    assert d0["list_slots"] == {0}                                     # the tail trip alone
    assert d1["list_trips"] == 24 and 128 in d1["totals"]              # one wave per element, exactly 128 hits, slots 0 and 1


@pytest.mark.parametrize("name", C.CASES)
def test_lattice_flavour_is_exact_in_any_order(name):
    c = C.case(name, "lattice")
    (e1, e2), (k1, k2), (S1, S2) = C.expected(name, "lattice")
    for x in (c.xyz1, c.xyz2, c.init1, c.init2) + tuple(C.terms(*t) for t in ((c.xyz1, c.xyz2, c.gd1, c.idx1), (c.xyz2, c.xyz1, c.gd2, c.idx2))):
        assert np.array_equal(x / C.QUANTUM, np.round(x / C.QUANTUM))
    # every partial sum of a row, in any order, is a whole number of quanta of magnitude <= S: exact below 2^24 quanta
    assert max(S1.max(), S2.max()) / C.QUANTUM < 2 ** 24, name
    assert np.array_equal(e1, e1.astype(np.float32)) and np.array_equal(e2, e2.astype(np.float32))
    assert int(k1.sum()) == c.bsz * c.m and int(k2.sum()) == c.bsz * c.n
    if name == "crowded_last_row":
        assert int(k2.max()) == 258048


def test_reference_counts_and_bound():
    """k and S on a hand-made call; the bound's formula."""
    a = np.array([[[1, 2, 3], [4, 6, 8]]], np.float32)
    b = np.array([[[0, 0, 1]]], np.float32)
    g1, g2 = np.array([[0.5, 0.25]], np.float32), np.array([[1.0]], np.float32)
    i1, i2 = np.zeros((1, 2), np.int32), np.ones((1, 1), np.int32)
    init1, init2 = np.full((1, 2, 3), 0.5, np.float32), np.full((1, 1, 3), -1.0, np.float32)
    (e1, e2), (k1, k2), (S1, S2) = C.reference(a, b, g1, g2, i1, i2, init1, init2)
    v1 = np.array([[1, 2, 2], [2, 3, 3.5]])           # 2 gd (a - b[0])
    v2 = np.array([-8, -12, -14.0])                   # 2 gd (b[0] - a[1])
    assert np.array_equal(e1[0], 0.5 + v1 + np.array([[0, 0, 0], -v2])) and np.array_equal(e2[0, 0], -1.0 + v2 - v1.sum(0))
    assert k1.reshape(-1).tolist() == [0, 1] and k2.reshape(-1).tolist() == [2]
    assert np.array_equal(S1[0], 0.5 + np.abs(v1) + np.array([[0, 0, 0], np.abs(v2)])) and np.array_equal(S2[0, 0], 1.0 + np.abs(v2) + v1.sum(0))
    u = 2.0 ** -24
    assert C.bound(3, 2.0) == 5 * u / (1 - 5 * u) * 2.0 and C.bound(0, 0.0) == 0.0


@pytest.mark.parametrize("name", C.SMALL + ("batch3", "batch8"))
def test_reference_agrees_with_the_pinned_oracle(oracle, name):
    """oracle.chamfer_backward is the reference's kernel summed sequentially in fp32 into zeroed gradients: within `bound` of
    `reference` on floats, equal to it on the lattice."""
    for flavour in ("float", "lattice"):
        c = C.case(name, flavour)
        zero1, zero2 = np.zeros_like(c.init1), np.zeros_like(c.init2)
        (e1, e2), (k1, k2), (S1, S2) = C.reference(c.xyz1, c.xyz2, c.gd1, c.gd2, c.idx1, c.idx2, zero1, zero2)
        o1, o2 = oracle.chamfer_backward(c.xyz1, c.xyz2, c.gd1, c.gd2, c.idx1, c.idx2)
        for o, e, k, S in ((o1, e1, k1, S1), (o2, e2, k2, S2)):
            if flavour == "lattice":
                assert np.array_equal(o.astype(np.float64), e), name
            else:
                assert (np.abs(o.astype(np.float64) - e) <= C.bound(k, S)).all(), name
                assert not np.array_equal(o.astype(np.float64), e) or name == "small_1_1_1"        # (the bound is not idle)
