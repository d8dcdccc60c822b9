"""The definition of a right farthest point sampling, stated plainly in the oracle (oracle_fps_minima, oracle_fps_check), and the
cases of tests/fps_check_cases.py held to it on the CPU: what tests/test_gpu_fps_check.py then asks of the device-side check
(csrc/fps_verify.hip) is decided here, by the reference alone."""
import collections

import numpy as np
import pytest

import fps_check_cases as C


@pytest.mark.parametrize("mode", [0, 1])
def test_fps_minima_draws_the_oracles_sequence(oracle, mode):
    """oracle.fps_minima's indices are oracle.fps's, and a recorded minimum is the sample's running minimum when it was drawn:
    the largest running minimum of the cloud after the earlier samples, +inf for the start point."""
    for cloud, x in C.clouds().items():
        n = len(x)
        idx, minima = oracle.fps_minima(x, n, mode)
        np.testing.assert_array_equal(idx, oracle.fps(x, n, mode), err_msg=cloud)
        assert minima[0] == np.inf and minima.dtype == np.float32
        for k in (1, max(1, n // 2)):          # (a shorter sampling is a prefix)
            i2, m2 = oracle.fps_minima(x, k, mode)
            np.testing.assert_array_equal(i2, idx[:k])
            np.testing.assert_array_equal(m2, minima[:k])
        for j in sorted(j for j in {1, n // 3, n - 1} if 1 <= j <= n - 1):
            D = C.running(cloud, mode, n, j)
            assert minima[j] == D.max() and idx[j] == int(np.argmax(D)), (cloud, j)
        assert (np.diff(minima[1:]) <= 0).all(), cloud          # (the running maximum never grows)


@pytest.mark.parametrize("mode", [0, 1])
def test_every_case_is_what_it_is_taken_for(oracle, mode):
    """The verdict is -1 exactly when (idx, minima[1:]) is oracle.fps_minima's; every mutant's first wrong step is the step that
    was mutated, every mutant differs from the right sequence in that step alone (kind 5: in that step and the next)."""
    cases = C.cases(mode)
    for tab in C.tables(mode):
        cases = cases + tab
    for c in cases:
        x = C.clouds()[c["cloud"]]
        ridx, rmin = oracle.fps_minima(x, c["k"], mode)
        same = np.array_equal(c["idx"], ridx) and np.array_equal(c["minima"][1:], rmin[1:])
        what = (c["cloud"], c["kind"], c["j"])
        assert c["expect"] == oracle.fps_check(x, c["idx"], c["minima"], mode)
        assert (c["expect"] == -1) == same, what
        assert same == (c["kind"] == 0), what
        if c["kind"]:
            assert c["expect"] == c["j"], what
            differ = np.flatnonzero((c["idx"] != ridx) | (c["minima"].view(np.int32) != rmin.view(np.int32)))
            assert set(differ) <= ({c["j"], c["j"] + 1} if c["kind"] == 5 else {c["j"]}), what
        if c["kind"] == 3:
            # self-consistent: the recorded minimum is the substituted point's own running minimum
            D = C.running(c["cloud"], mode, c["k"], c["j"])
            assert c["minima"][c["j"]] == D[c["idx"][c["j"]]] and c["idx"][c["j"]] != ridx[c["j"]], what
            assert ridx[c["j"]] in c["witness"] and (D[list(c["witness"])] == rmin[c["j"]]).all(), what
        if c["kind"] == 4:
            assert c["witness"] == (int(ridx[c["j"]]),) and c["minima"][c["j"]] == rmin[c["j"]], what


def test_every_kind_has_a_case_in_every_position_class():
    have = collections.Counter()
    witnesses = set()
    kinds = collections.Counter()
    for mode in (0, 1):
        per_mode = collections.Counter()
        for c in C.cases(mode):
            kinds[c["kind"]] += 1
            for cls in c["cls"]:
                per_mode[(c["kind"], cls)] += 1
            if c["kind"] in (3, 4):
                n = len(C.clouds()[c["cloud"]])
                for w in c["witness"]:
                    witnesses |= {str(w)} & {"0", "127", "128"}
                    if w == n - 1 and n % C.BLOCK:
                        witnesses.add("n-1")
        missing = [(kind, cls) for kind in C.POSITION_KINDS for cls in C.CLASSES if not per_mode[(kind, cls)]]
        assert not missing, (mode, missing)
        have += per_mode
    assert witnesses == set(C.WITNESS_POINTS), witnesses
    assert all(kinds[kind] > 0 for kind in range(10)), kinds
    # kind 4 on a lattice (not only among the repeated points' zeros) in every class a lattice has steps in
    for mode in (0, 1):
        lat = {cls for c in C.cases(mode) if c["kind"] == 4 and c["cloud"].startswith("lattice") for cls in c["cls"]}
        assert lat >= set(C.CLASSES) - {"seg1"}, (mode, sorted(lat))
    print("cases per kind (both modes):", dict(sorted(kinds.items())))


def test_the_clouds_and_positions_are_the_ones_named():
    cl = C.clouds()
    assert [len(cl["uniform%d" % n]) for n in C.UNIFORM] == list(C.UNIFORM)
    lat = cl["lattice512"]
    assert len(lat) == 512 and len(np.unique(lat, axis=0)) == 512 and np.array_equal(lat * 8, np.round(lat * 8))
    d = cl["dups%d" % C.DUPS_N]
    assert len(np.unique(d, axis=0)) == C.DUPS_N - C.DUPS_REPEATED
    assert C.per_of(1300, 1) == 1304 and C.per_of(1300, 2) == 656 and C.per_of(9, 16) == 8 and C.per_of(1, 3) == 0
    pos = C.positions(1300)
    assert {1, 7, 8, 9, 655, 656, 657, 1023, 1024, 1025, 1298, 1299} <= set(pos)
    assert pos[1024] == {"tile"} and pos[1299] == {"tail"} and "seg16" in pos[88]
    # the job tables: eight clouds of different n and k, the mutant in one slot
    for mode in (0, 1):
        tabs = C.tables(mode)
        assert len(tabs) == 9 and all(len(t) == 8 for t in tabs)
        assert len({(len(cl[c["cloud"]]), c["k"]) for c in tabs[0]}) == 8
        assert [[c["expect"] >= 0 for c in t] for t in tabs[1:]] == [[s == q for s in range(8)] for q in range(8)]
        assert all(c["expect"] == -1 for c in tabs[0])
