"""tests/nn_seeded_cases.py builds what it says (no GPU): the properties of the inputs that tests/test_gpu_nn_seeded.py relies
on, shown with the oracle alone -- oracle.pose_transform stands in for the posed cloud the GPU returns (equal to 3e-7; on the
lattice exactly).  Ties are detected with the oracle itself: chamfer_forward against the targets in reversed order; a query
whose two answers map to different original indices has a tie."""
import os
import re

import numpy as np
import pytest

import nn_seeded_cases as C

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "genpc_amd", "csrc")
MODES = (0, 1)


def _constant(path, name):
    m = re.search(r"\b%s\s*=\s*(\d+)\s*;" % name, open(os.path.join(CSRC, path)).read())
    assert m, (path, name)
    return int(m.group(1))


def _posed(case):
    return C.posed_by_oracle(case[0], case[1], case[2])


def _copies(targets):
    """[nt] int: how many targets have exactly this target's bits"""
    rows = np.ascontiguousarray(targets).view(np.uint32).reshape(-1, 3)
    _, inv, cnt = np.unique(rows, axis=0, return_inverse=True, return_counts=True)
    return cnt[inv.reshape(-1)]


def test_what_the_kernel_constants_are():
    """The numbers the case module restates or the sizes rest on, read from the code."""
    assert _constant("nn_plan.h", "kBlock") // _constant("nn_seeded.hip", "kSLPQ") == C.QUERIES_PER_BLOCK
    clamp = _constant("grid.h", "kCellGridMaxCells") * 3 // 4
    assert C.CAP_NM // 2 > clamp and C.CAP_NS // 2 > clamp           # build_seeded_grids: target(n) = n / 2, clamped
    rest, _, _, stat = C.case("cap", "loop")
    assert rest.shape == (1, C.CAP_NM, 3) and stat.shape == (1, C.CAP_NS, 3)
    # the sampled launch's case: direction 2 does not start on a multiple of kPoseSample blocks
    sample = _constant("pose.hip", "kPoseSample")
    nm = C.case("ellipsoid1100", "loop")[0].shape[1]
    _, blocks0 = C.sampled_mask(3, nm, 0, sample)
    assert sample > 1 and blocks0 % sample != 0


def test_sizes_are_no_multiples_of_the_block():
    for cloud in ("ellipsoid", "ellipsoid65", "ellipsoid1100", "cap", "far_origin", "scale_1e-3", "scale_1e3", "batch3"):
        rest, _, _, stat = C.case(cloud, "loop")
        assert rest.shape[1] % C.QUERIES_PER_BLOCK and stat.shape[1] % C.QUERIES_PER_BLOCK, cloud
    assert [C.case("tiny_%d_%d" % s, "loop")[k].shape[1] for s in ((1, 1), (1, 5), (5, 1), (7, 3)) for k in (0, 3)] == [1, 1, 1, 5, 5, 1, 7, 3]
    assert C.case("duplicates", "loop")[3].shape[1] == 1024


@pytest.mark.parametrize("cloud", C.POSED_CLOUDS)
def test_every_pose_leaves_finite_points(cloud):
    """... the poses for which the kernel must give up culling included; they are what they say."""
    for name in C.POSES:
        case = C.case(cloud, name)
        assert all(np.isfinite(a).all() for a in case), (cloud, name)
        assert np.isfinite(_posed(case)).all(), (cloud, name)
        assert np.isfinite(_posed(case[:2] + (np.stack([C.moved(p) for p in case[2]]),))).all(), (cloud, name)
    size = C.size_of(C.case(cloud, "loop")[0][0])
    a1, a2 = C.pose("unnormalised", size)[0:3].astype(np.float64), C.pose("unnormalised", size)[3:6].astype(np.float64)
    assert abs(np.linalg.norm(a1) - 5.0) < 1e-5 and abs(a1 @ a2 / np.linalg.norm(a1) / np.linalg.norm(a2) - 0.5) < 1e-6
    p = C.pose("parallel", size)
    assert np.array_equal(p[3:6], 2 * p[0:3]) and not C.pose("a1_zero", size)[0:3].any()
    assert np.exp(np.float32(50.0)) > 1e20 and np.exp(np.float32(-50.0)) < 1e-20          # the kernel's range of s for culling
    assert np.abs(C.pose("far_translation", size)[6:9]).max() >= 30 * size
    R170 = C.R_170
    assert abs(np.degrees(np.arccos((np.trace(R170) - 1) / 2)) - 170.0) < 1e-9


def test_degenerate_clouds_reach_the_grid_size_branches():
    """flat / line / point: 2, 1 and 0 axes with an extent -- the rest cloud under every pose, the static cloud too under the
    identity (it is cut from the posed cloud; a rotation tilts it)."""
    for cloud, nact in (("flat", 2), ("line", 1), ("point", 0)):
        for name in C.POSES:
            rest = C.case(cloud, name)[0][0]
            assert int(((rest.max(0) - rest.min(0)) > 0).sum()) == nact, (cloud, name)
        stat = C.case(cloud, "identity")[3][0]
        assert int(((stat.max(0) - stat.min(0)) > 0).sum()) == nact, cloud
    far = C.case("far_origin", "loop")[0][0]
    assert np.abs(far.mean(0)).min() > 400


def test_lattice_is_posed_onto_itself_and_ties(oracle):
    rest, center, params, stat, expect = C.lattice()
    posed = _posed((rest, center, params))
    assert np.array_equal(posed, expect)
    as_set = lambda a: set(map(tuple, a.reshape(-1, 3).tolist()))
    assert as_set(expect) == as_set(rest) and len(as_set(rest)) == 729 and len(as_set(stat)) == 512
    in1, in2 = C.interior(posed[0], stat[0]), C.interior(stat[0], posed[0])
    assert in1.mean() >= 0.5 and in2.mean() >= 0.5
    assert int(in1.sum()) == 343 + 6 * 49 and int(in2.sum()) == 512
    for mode in MODES:
        d1, i1, d2, i2 = C.answers(oracle, posed, stat, mode)
        h1, h2 = C.highest_minima(oracle, posed, stat, mode)
        assert (h1[0][in1] != i1[0][in1]).all() and (h2[0][in2] != i2[0][in2]).all(), mode
        assert (d2 == np.float32(0.75)).all() and (d1[0][in1] == np.float32(0.75)).all()
        # tie_high differs from the oracle's answer on at least half of each direction
        s1, s2 = C.seeds("tie_high", oracle, posed, stat, mode)
        assert (s1 != i1).mean() >= 0.5 and (s2 != i2).mean() >= 0.5
        assert (s1 >= i1).all() and (s2 >= i2).all()


@pytest.mark.parametrize("name", [p for p in C.POSES if p not in ("ls_plus50", "ls_minus50")])
def test_duplicates_are_answers(oracle, name):
    """At least a quarter of the queries of each direction have a nearest target that exists in two or more copies, and for
    those tie_high names another index than the oracle.  (Not at log s = +/-50: there every squared distance overflows to +inf
    or underflows to 0, all targets tie and the answer is target 0 whatever is duplicated.)"""
    case = C.case("duplicates", name)
    posed, stat = _posed(case), case[3]
    c_stat, c_posed = _copies(stat[0]), _copies(posed[0])
    for mode in MODES:
        d1, i1, d2, i2 = C.answers(oracle, posed, stat, mode)
        dup1, dup2 = c_stat[i1[0]] >= 2, c_posed[i2[0]] >= 2
        print("duplicates %-16s mode %d: nearest target duplicated for %.3f / %.3f of the queries" % (name, mode, dup1.mean(), dup2.mean()))
        assert dup1.mean() >= 0.25 and dup2.mean() >= 0.25, (name, mode)
        s1, s2 = C.seeds("tie_high", oracle, posed, stat, mode)
        assert (s1[0][dup1] > i1[0][dup1]).all() and (s2[0][dup2] > i2[0][dup2]).all()
        assert (s1 != i1).mean() >= 0.25 and (s2 != i2).mean() >= 0.25


def test_seed_policies_are_what_they_say(oracle):
    case = C.case("ellipsoid", "loop")
    rest, center, params, stat = case
    posed = _posed(case)
    nm, ns = rest.shape[1], stat.shape[1]
    ex = C.answers(oracle, posed, stat, 1)
    got = {p: C.seeds(p, oracle, posed, stat, 1, rest, center, params, exact=ex) for p in C.POLICIES}
    for p, (s1, s2) in got.items():
        assert s1.shape == (1, nm) and s2.shape == (1, ns) and s1.dtype == np.int32 and s2.dtype == np.int32, p
    assert (got["none"][0] == -1).all() and (got["none"][1] == -1).all()
    for s, nt in zip(got["out_of_range"], (ns, nm)):
        assert set(np.unique(s).tolist()) == {nt, nt + 7, C.INT_MIN}
    for p in ("exact", "farthest", "random", "previous_step", "tie_high"):
        for s, nt in zip(got[p], (ns, nm)):
            assert s.min() >= 0 and s.max() < nt, p
    assert np.array_equal(got["exact"][0], ex[1]) and np.array_equal(got["exact"][1], ex[3])
    # the farthest target is far: farther than the cloud's half size; a step-old answer is mostly, not always, still right
    far = np.linalg.norm(posed[0] - stat[0][got["farthest"][0][0]], axis=1)
    assert far.min() > 0.5 * C.size_of(rest[0]) * 0.9
    same = (got["previous_step"][0] == ex[1]).mean()
    print("previous_step: %.3f of direction 1's seeds are still the answer" % same)
    assert 0.3 < same < 1.0
    # the reversed run reports the same distances: its index is one of the bit-equal minima
    r = C.answers(oracle, posed, np.ascontiguousarray(stat[:, ::-1]), 1)
    assert np.array_equal(r[0].view(np.uint32), ex[0].view(np.uint32))


def test_batch3_elements_do_not_share_a_pose():
    rest, center, params, stat = C.case("batch3", "loop")
    assert rest.shape == (3, 1000, 3) and stat.shape == (3, 777, 3)
    for a in (rest, center, params, stat):
        assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[1], a[2]) and not np.array_equal(a[0], a[2])


def test_sampled_mask_numbers_blocks_across_directions():
    m, blocks0 = C.sampled_mask(3, 130, 0, 4)          # 3 blocks per element: blocks 0, 4, 8 -> element 0 block 0, 1 block 1, 2 block 2
    assert blocks0 == 9
    assert m[0, :64].all() and not m[0, 64:].any() and m[1, 64:128].all() and not m[1, :64].any() and m[2, 128:].all() and not m[2, :128].any()
    m2, _ = C.sampled_mask(1, 64, blocks0, 4)          # direction 2 starts at block 9: not answered
    assert not m2.any()
