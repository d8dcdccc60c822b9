"""tests/grid_cases.py has teeth (no GPU): on its cases a numpy-fp32 restatement of grid.h's cell function, gap and cell range
keeps both claims exactly, and each of three small mutations of that arithmetic -- no slack in the gap, the range's slack
with the wrong sign, round to nearest for floor -- breaks a claim on at least one case of the family named below.  A family
that lets a mutant through is too weak for tests/test_gpu_grid.py, which runs the same cases through the device's own helpers."""
import numpy as np
import pytest

import grid_cases as G


@pytest.fixture(scope="module")
def cases():
    return G.bound_cases()


def test_cases_are_deterministic_and_within_the_sizes():
    a, b = G.bound_cases(), G.bound_cases()
    assert [c["name"] for c in a] == [c["name"] for c in b]
    for x, y in zip(a, b):
        assert x["p"].tobytes() == y["p"].tobytes() and x["q"].tobytes() == y["q"].tobytes()
        assert len(x["p"]) <= 4096 and len(x["q"]) <= 256, x["name"]
        assert (x["frame"].g >= 2).all() and ((x["frame"].g <= 64) | (x["frame"].g == 1024)).all()
    assert sum(1 for c in a if (c["frame"].g == 1024).any()) == 1
    assert {c["name"].split()[0] for c in a} == {"walls", "far", "scale", "ties"}


def test_restated_claims_hold_on_every_case(cases):
    for c in cases:
        F, p, q = c["frame"], c["p"], c["q"]
        assert G.gap_violations(F, p, q) == 0, c["name"]
        assert G.gap_violations(F, p, q, w=4) == 0, c["name"]
        assert G.range_violations(F, p[::7], q) == 0, c["name"]
        if c["mn"] is not None:           # the icp.hip form: the cloud's exact minimum and maximum for outer walls
            assert (F.lo == c["mn"]).all() and (p >= c["mn"]).all() and (p <= c["mx"]).all()
            assert G.gap_violations(F, p, q, mn=c["mn"], mx=c["mx"]) == 0, c["name"]


def test_without_slack_the_wall_family_breaks_the_gap_claim():
    gap_bad = sum(G.gap_violations(c["frame"], c["p"], c["q"], slack_scale=0) for c in G.walls())
    assert gap_bad > 0


def test_range_claim_needs_no_slack_but_breaks_when_it_is_applied_inwards():
    """The range claim is stated for a radius with |p_a - q_a| <= R EXACTLY.  Then q - R <= p exactly, rounding to nearest is
    monotone and leaves the fp32 value p where it is, so fl(q - R) <= p, and the cell function is a chain of monotone steps:
    cell(fl(q - R)) <= cell(p) with no slack at all (the same at the upper end).  No input can violate it at slack_scale = 0
    -- the slack of grid_cell_range is room for radii that are only nearly upper bounds -- and this test pins that rather than
    look for a violation that cannot exist.  The family's teeth show on the neighbouring mistake, the slack applied with the
    wrong sign (slack_scale = -1: the range shrinks by it at either end)."""
    none = inwards = 0
    for c in G.walls():
        none += G.range_violations(c["frame"], c["p"][::7], c["q"], slack_scale=0)
        inwards += G.range_violations(c["frame"], c["p"][::7], c["q"], slack_scale=-1)
    assert none == 0
    assert inwards > 0


def test_round_to_nearest_breaks_the_gap_claim():
    """a point of the upper half of a cell is sorted one cell up, half a cell beyond that cell's wall: no slack covers it"""
    per_family = {}
    for c in G.bound_cases():
        fam = c["name"].split()[0]
        per_family[fam] = per_family.get(fam, 0) + G.gap_violations(c["frame"], c["p"], c["q"], rnd=np.rint)
    assert per_family["far"] > 0 and per_family["scale"] > 0, per_family     # the families with points inside the cells


def test_exact_checker_is_exact():
    """the float64 shortcut is taken only where it is exact; elsewhere the Fraction path decides"""
    p = np.array([1.0, 1e-45, 16777216.0, 3e38], np.float32)
    q = np.array([1.0 + 2.0 ** -23, 10.0, 1.0, -3e38], np.float32)
    d, inexact = G.exact_absdiff(p, q)
    assert list(inexact) == [False, True, False, False]      # 10 - 1e-45 needs 150 bits; 6e38 is a float64
    assert d[0] == 2.0 ** -23 and d[2] == 16777215.0
    assert list(G.le_absdiff(np.float32([2.0 ** -23, 10.0, 16777216.0, 0.0]), p, q)) == [True, False, False, True]
    assert list(G.within(p, q, np.float32([2.0 ** -23, 10.0, 16777215.0, np.inf]))) == [True, True, True, True]
    assert list(G.within(p, q, np.float32([2.0 ** -24, 9.999999, 16777214.0, 3e38]))) == [False, False, False, False]


def test_nonfinite_queries_restated():
    q, want = G.nonfinite_queries()
    F = G.Frame((-0.5, 0.0, 1e3), 0.25, (7, 64, 2))
    for row, a, w in want:
        c = int(G.cell1(q[row, a], F.lo[a], F.inv, F.g[a]))
        assert c == (0 if w == "0" else int(F.g[a]) - 1), (row, a, w)


def test_degenerate_clouds_and_boxes_are_what_their_names_say():
    d = dict(G.degenerate())
    assert len(np.unique(d["identical"], axis=0)) == 1
    assert len(np.unique(d["plane"][:, 1])) == 1 and len(np.unique(d["line"][:, 0])) == 1 and len(np.unique(d["line"][:, 2])) == 1
    assert len(d["n=1"]) == 1 and len(d["n=1025"]) == 1025
    assert np.isnan(d["one NaN"]).sum() == 1 and np.isinf(d["one inf"]).sum() == 1
    with np.errstate(over="ignore"):
        assert np.isinf(d["extent overflows"][:, 0].max() - d["extent overflows"][:, 0].min())
    assert all(len(v) <= 4096 for v in d.values())
    assert len(G.size_boxes()) >= 10
