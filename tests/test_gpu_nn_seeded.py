"""nn_seeded_kernel (csrc/nn_seeded.hip), the loop's nearest-neighbour search from the second Adam step on, query by query
against the reference: genpc_nn_seeded_step runs ONE seeded step with the loop's own functions on the inputs of
tests/nn_seeded_cases.py, and (d1, i1, d2, i2) must equal oracle.chamfer_forward(posed, stat, mode) on the posed cloud the GPU
returned BIT FOR BIT -- distances compared as uint32, indices as int32, no tolerance anywhere -- in both arithmetic modes.
tests/test_nn_seeded_cases.py shows on the CPU that the inputs have the ties, duplicates and degenerate extents claimed here.

Poses: identity, the loop's regime, 170 degrees, log s = +/-2, unnormalised parameters, a translation of 50 and of 1e6 cloud
sizes, and four for which the kernel must give up culling (nn_seeded_cases.POSES).
What is run (the full product cloud x pose x policy would be ~5000 steps and as many oracle calls; kept instead):
  * every seed policy for `ellipsoid` (1000 / 777 and 65 / 63), `duplicates`, `batch3` under every pose, and for `lattice`;
  * every pose under the policies `exact` and `none` for the rest: tiny, flat, line, point, far_origin, both scales, cap and
    the 1100 / 777 ellipsoid of the sampled launch.
The seeds of a step are made from the oracle's answers ON THAT STEP'S posed cloud (`exact` is exact, `tie_high` is the highest
of the bit-equal minima), `previous_step` from the oracle's answers at the pose a step earlier.
The reference of a (cloud, pose, mode) is computed once and shared by the tests of this file.

What the file was seen to catch, each as a one-line change of nn_seeded.hip on a scratch copy:
  * the row test `lb > rg2` made `>=`: 22 cases fail, all at log s = +/-50 and translation_1e6, where squared distances are 0
    or +inf and the bound EQUALS the best distance (elsewhere grid.h's slack keeps the bound below it, ties included);
  * the merge comparing distances only: 136 cases fail (lattice, duplicates, repeated steps, every pose of the clouds with
    exact ties);
  * the moving grid's margins removed (rel = 1, dg = 0): the 6 cases at translation_1e6 fail (ties at distance 0 in other
    cells than the seed's) -- nothing at the loop's own magnitudes reaches that margin;
  * the slack terms dropped from the box bounds: NOTHING here fails.  They cover the rounding of the cell function, ~1e-7 of a
    cell, under a box already widened by 1e-6 of its radius; no case of this file puts a target that close to a cell wall
    with the ball's edge on the other side of it.
It also found one wrong answer, fixed with it: a seed whose distance overflowed to +inf made a row's width NaN -> 0 (log s = 50)."""
import contextlib
import ctypes
import os
import re

import numpy as np
import pytest

import nn_seeded_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MODES = (0, 1)
SENTINEL_D, SENTINEL_I = np.float32(-12345.5), np.int32(-7)          # (-7: outside every target count, so no seed either)


@pytest.fixture(scope="module")
def gp():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib, chamfer_3D
    from genpc_amd.optim_registration import diff_obj_pose as POSE
    return dict(torch=torch, POSE=POSE, L=_lib, lib=_lib.lib, chamfer=chamfer_3D)


@contextlib.contextmanager
def arith(gp, mode):
    """The arithmetic mode (process default, no thread override) and nn_forward's default dispatch; restored afterwards."""
    prev_state = gp["L"].thread_state()
    st = list(prev_state[0])
    st[0], st[1], st[2] = -1, -1, 0
    prev_mode = gp["lib"].genpc_set_arith(mode)
    gp["L"].apply_thread_state((tuple(st), prev_state[1]))
    try:
        yield
    finally:
        gp["L"].apply_thread_state(prev_state)
        gp["lib"].genpc_set_arith(prev_mode)


_DEV = {}


def _dev(gp, case):
    """The four input arrays of a case on the device, uploaded once per array (the case module hands out the same objects)."""
    out = []
    for a in case[:4]:
        if id(a) not in _DEV:
            _DEV[id(a)] = (a, gp["torch"].from_numpy(np.array(a)).cuda())
        out.append(_DEV[id(a)][1])
    return out


def step(gp, case, seed1, seed2, sample=1, d1=None, d2=None):
    """One seeded step -> (posed, d1, i1, d2, i2) as numpy arrays."""
    torch = gp["torch"]
    rest, center, params, stat = _dev(gp, case)
    up = lambda a: None if a is None else torch.from_numpy(np.array(a)).cuda()
    out = gp["POSE"].nn_seeded_step(rest, center, params, stat, up(seed1), up(seed2), sample=sample, d1=up(d1), d2=up(d2))
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def brute_force(gp, posed, stat):
    """genpc_chamfer_forward on the device -> (d1, i1, d2, i2)"""
    torch = gp["torch"]
    p, s = torch.from_numpy(np.array(posed)).cuda(), torch.from_numpy(np.array(stat)).cuda()
    b, n, m = p.shape[0], p.shape[1], s.shape[1]
    d1, d2 = torch.empty(b, n, device="cuda"), torch.empty(b, m, device="cuda")
    i1, i2 = torch.empty(b, n, device="cuda", dtype=torch.int32), torch.empty(b, m, device="cuda", dtype=torch.int32)
    assert gp["chamfer"].forward(p, s, d1, d2, i1, i2) == 1, gp["L"].last_error()
    torch.cuda.synchronize()
    return d1.cpu().numpy(), i1.cpu().numpy(), d2.cpu().numpy(), i2.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def differences(tag, got, want):
    """got, want = (d1, i1, d2, i2).  Prints, per direction that differs: the case, the direction, the number of differing
    queries and the first of them with both (distance bits, index) pairs.  -> the number of differing queries."""
    total = 0
    for k, name in ((0, "direction 1 (posed -> static)"), (2, "direction 2 (static -> posed)")):
        gd, gi, wd, wi = bits(got[k]), np.asarray(got[k + 1], np.int32), bits(want[k]), np.asarray(want[k + 1], np.int32)
        assert gd.shape == wd.shape and gi.shape == wi.shape, (tag, name, gd.shape, wd.shape)
        bad = np.argwhere((gd != wd) | (gi != wi))
        if len(bad):
            f = tuple(bad[0])
            print("%s: %s: %d of %d queries differ; first: element %d query %d  got (0x%08x, %d)  reference (0x%08x, %d)"
                  % (tag, name, len(bad), gd.size, f[0], f[1], gd[f], gi[f], wd[f], wi[f]))
        total += len(bad)
    return total


_REF = {}


def reference(gp, oracle, key, case, mode):
    """-> (posed as the GPU returns it, the oracle's (d1, i1, d2, i2) on it); one unseeded step and one oracle call per key.
    Call inside arith(gp, mode)."""
    key = key + (mode,)
    if key not in _REF:
        none = C.seeds("none", oracle, case[0], case[3], mode)
        posed = step(gp, case, *none)[0]
        ans = C.answers(oracle, posed, case[3], mode)
        for a in (posed,) + ans:
            a.setflags(write=False)
        _REF[key] = (posed, ans)
    return _REF[key]


def run_policies(gp, oracle, key, case, mode, policies):
    """Every policy's step equals the oracle and returns the same posed cloud; -> {policy: outputs}."""
    posed, ans = reference(gp, oracle, key, case, mode)
    rest, center, params, stat = case
    wrong, outs = [], {}
    for policy in policies:
        s1, s2 = C.seeds(policy, oracle, posed, stat, mode, rest, center, params, exact=ans)
        out = step(gp, case, s1, s2)
        assert np.array_equal(bits(out[0]), bits(posed)), (key, mode, policy, "the posed cloud depends on the seeds")
        if differences("%s mode %d seeds %s" % ("/".join(map(str, key)), mode, policy), out[1:], ans):
            wrong.append(policy)
        outs[policy] = out
    assert not wrong, (key, mode, wrong)
    return outs


def policies_of(cloud):
    return C.POLICIES if cloud in C.ALL_POLICY_CLOUDS else C.CHEAP_POLICIES


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pose", C.POSES)
@pytest.mark.parametrize("cloud", C.POSED_CLOUDS)
def test_equals_the_oracle(gp, oracle, cloud, pose, mode):
    with arith(gp, mode):
        run_policies(gp, oracle, (cloud, pose), C.case(cloud, pose), mode, policies_of(cloud))


@pytest.mark.parametrize("mode", MODES)
def test_lattice_equals_the_oracle_under_every_policy(gp, oracle, mode):
    """Exact ties: every cell centre has eight equidistant lattice points, the ball of a tie_high seed passes exactly through
    them in several cells and rows, and the lowest index must still come out.  The premise first: the posed lattice IS the
    lattice."""
    rest, center, params, stat, expect = C.lattice()
    case = (rest, center, params, stat)
    with arith(gp, mode):
        posed, ans = reference(gp, oracle, ("lattice", "lattice"), case, mode)
        assert np.array_equal(posed, expect)
        assert (ans[2] == np.float32(0.75)).all()
        run_policies(gp, oracle, ("lattice", "lattice"), case, mode, C.POLICIES)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cloud,pose", [("ellipsoid", "loop"), ("ellipsoid", "rot170"), ("duplicates", "loop"), ("lattice", "lattice")])
def test_seed_independence(gp, oracle, cloud, pose, mode):
    """All seed policies give byte-identical outputs."""
    case = C.lattice()[:4] if cloud == "lattice" else C.case(cloud, pose)
    with arith(gp, mode):
        outs = run_policies(gp, oracle, (cloud, pose), case, mode, C.POLICIES)
    first = outs[C.POLICIES[0]]
    for policy, out in outs.items():
        for a, b_ in zip(out, first):
            assert a.tobytes() == b_.tobytes(), (cloud, pose, mode, policy)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pose", C.POSES)
@pytest.mark.parametrize("cloud", ("ellipsoid", "duplicates", "cap"))
def test_agrees_with_the_brute_force_filter(gp, oracle, cloud, pose, mode):
    """genpc_chamfer_forward on the same posed cloud gives the same bytes: what the loop's mode switch assumes."""
    case = C.case(cloud, pose)
    with arith(gp, mode):
        posed, ans = reference(gp, oracle, (cloud, pose), case, mode)
        s1, s2 = C.seeds("exact", oracle, posed, case[3], mode, exact=ans)
        out = step(gp, case, s1, s2)
        bf = brute_force(gp, posed, case[3])
    assert differences("%s/%s mode %d seeded vs genpc_chamfer_forward" % (cloud, pose, mode), out[1:], bf) == 0
    assert differences("%s/%s mode %d genpc_chamfer_forward vs oracle" % (cloud, pose, mode), bf, ans) == 0


@pytest.mark.parametrize("mode", MODES)
def test_batch_isolation(gp, oracle, mode):
    """batch3 equals its three elements run one at a time; swapping the poses of elements 0 and 2 changes only their outputs."""
    case = C.case("batch3", "loop")
    with arith(gp, mode):
        whole = run_policies(gp, oracle, ("batch3", "loop"), case, mode, ("random",))["random"]
        s1, s2 = C.seeds("random", oracle, whole[0], case[3], mode)
        for e in range(3):
            one = tuple(np.ascontiguousarray(a[e:e + 1]) for a in case)
            alone = step(gp, one, s1[e:e + 1], s2[e:e + 1])
            for a, b_ in zip(alone, whole):
                assert a.tobytes() == b_[e:e + 1].tobytes(), (mode, e)
        swapped_params = np.ascontiguousarray(case[2][[2, 1, 0]])
        swapped = step(gp, (case[0], case[1], swapped_params, case[3]), s1, s2)
        want = C.answers(oracle, swapped[0], case[3], mode)
        assert differences("batch3 with the poses of elements 0 and 2 swapped, mode %d" % mode, swapped[1:], want) == 0
    for a, b_ in zip(swapped, whole):
        assert a[1].tobytes() == b_[1].tobytes(), mode
    for e in (0, 2):
        assert not np.array_equal(swapped[0][e], whole[0][e]) and not np.array_equal(swapped[1][e], whole[1][e]), (mode, e)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cloud", ("ellipsoid", "duplicates"))
def test_repeated_steps(gp, oracle, cloud, mode):
    """The loop's use: a call's outputs are the next call's seeds at a pose moved by lr = 0.01, ten times; each step equals
    the oracle -- per step and per query, not through a sum."""
    rest, center, params, stat = C.case(cloud, "loop")
    with arith(gp, mode):
        s1, s2 = C.seeds("none", oracle, rest, stat, mode)
        wrong = 0
        for k in range(11):
            posed, d1, i1, d2, i2 = step(gp, (rest, center, params, stat), s1, s2)
            want = C.answers(oracle, posed, stat, mode)
            wrong += differences("%s step %d mode %d" % (cloud, k, mode), (d1, i1, d2, i2), want)
            if k:
                print("%s step %d mode %d: %.3f / %.3f of the seeds were still the answer" % (cloud, k, mode, (s1 == i1).mean(), (s2 == i2).mean()))
            s1, s2 = i1, i2
            params = np.stack([C.moved(p) for p in params])
        assert wrong == 0


def pose_sample():
    """PoseProbe::kPoseSample, read from the loop's source."""
    m = re.search(r"\bkPoseSample\s*=\s*(\d+)\s*;", open(os.path.join(ROOT, "genpc_amd", "csrc", "pose.hip")).read())
    return int(m.group(1))


@pytest.mark.parametrize("mode", MODES)
def test_sampled_launch(gp, oracle, mode):
    """sample = kPoseSample (the loop's timing probe): exactly the queries of every sample-th block of 64, numbered across both
    directions as launch_nn_seeded numbers them, carry the full call's answers; all others still hold what they held.
    3 x 1100 posed points are 54 blocks: direction 2 starts on no multiple of the sample."""
    sample = pose_sample()
    parts = [C.case("ellipsoid1100", p) for p in C.BATCH3_POSES]
    case = tuple(np.ascontiguousarray(np.concatenate([p[k] for p in parts])) for k in range(4))
    b, nm, ns = case[0].shape[0], case[0].shape[1], case[3].shape[1]
    m1, blocks0 = C.sampled_mask(b, nm, 0, sample)
    m2, _ = C.sampled_mask(b, ns, blocks0, sample)
    assert sample > 1 and blocks0 % sample != 0
    assert 0 < m1.sum() < m1.size and 0 < m2.sum() < m2.size
    fill = lambda shape, v: np.full(shape, v, dtype=v.dtype)
    with arith(gp, mode):
        full = run_policies(gp, oracle, ("ellipsoid1100x3", "batch3 poses"), case, mode, ("none",))["none"]
        got = step(gp, case, fill((b, nm), SENTINEL_I), fill((b, ns), SENTINEL_I), sample=sample,
                   d1=fill((b, nm), SENTINEL_D), d2=fill((b, ns), SENTINEL_D))
    assert np.array_equal(bits(got[0]), bits(full[0]))
    for k, mask in ((1, m1), (3, m2)):
        d, i = got[k], got[k + 1]
        assert np.array_equal(bits(d)[mask], bits(full[k])[mask]) and np.array_equal(i[mask], full[k + 1][mask]), (mode, k)
        assert (bits(d)[~mask] == bits(SENTINEL_D)).all() and (i[~mask] == SENTINEL_I).all(), (mode, k)


def test_refusals(gp):
    """Bad counts and sample = 0: -1, genpc_last_error says who refused, nothing is written.  (Straight through the C entry
    point: the wrapper takes its counts from the tensors' shapes and cannot express them.)"""
    torch, lib, p = gp["torch"], gp["lib"], gp["L"].ptr
    rest, center, params, stat = _dev(gp, C.case("tiny_7_3", "loop"))
    null = ctypes.c_void_p(0)
    for b, nm, ns, sample in ((0, 7, 3, 1), (-1, 7, 3, 1), (1, 0, 3, 1), (1, -5, 3, 1), (1, 7, 0, 1), (1, 7, -2, 1), (1, 7, 3, 0), (1, 7, 3, -4)):
        posed = torch.full((1, 7, 3), float(SENTINEL_D), device="cuda")
        d1, d2 = torch.full((1, 7), float(SENTINEL_D), device="cuda"), torch.full((1, 3), float(SENTINEL_D), device="cuda")
        i1 = torch.full((1, 7), int(SENTINEL_I), device="cuda", dtype=torch.int32)
        i2 = torch.full((1, 3), int(SENTINEL_I), device="cuda", dtype=torch.int32)
        assert lib.genpc_fps_tune(1) == -1 and "genpc_fps_tune" in gp["L"].last_error()          # (another refusal's message first)
        rc =lib.genpc_nn_seeded_step(b, nm, p(rest), p(center), p(params), ns, p(stat), p(posed), p(d1), p(i1), p(d2), p(i2), sample, null)
        torch.cuda.synchronize()
        assert rc == -1, (b, nm, ns, sample, rc)
        assert "genpc_nn_seeded_step" in gp["L"].last_error(), (b, nm, ns, sample, gp["L"].last_error())
        for t in (posed, d1, d2):
            assert (t == float(SENTINEL_D)).all(), (b, nm, ns, sample)
        for t in (i1, i2):
            assert (t == int(SENTINEL_I)).all(), (b, nm, ns, sample)
    with pytest.raises(ValueError):
        gp["POSE"].nn_seeded_step(rest, center, params[:, :9].contiguous(), stat, i1, i2)
    with pytest.raises(ValueError):
        gp["POSE"].nn_seeded_step(rest, center, params, stat, i2, i1)
    with pytest.raises(TypeError):
        gp["POSE"].nn_seeded_step(rest, center, params, stat, i1.float(), i2)
    with pytest.raises(RuntimeError, match="rc=-1"):
        gp["POSE"].nn_seeded_step(rest, center, params, stat, i1, i2, sample=0)


@pytest.mark.parametrize("mode", MODES)
def test_non_default_stream(gp, oracle, mode):
    """The same bytes on a stream of the caller's as on the default stream (grids, transform and search all follow it)."""
    torch = gp["torch"]
    case = C.case("ellipsoid", "rot170")
    with arith(gp, mode):
        posed, ans = reference(gp, oracle, ("ellipsoid", "rot170"), case, mode)
        s1, s2 = C.seeds("random", oracle, posed, case[3], mode)
        on_default = step(gp, case, s1, s2)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            on_side = step(gp, case, s1, s2)
        side.synchronize()
    for a, b_ in zip(on_side, on_default):
        assert a.tobytes() == b_.tobytes(), mode
    assert differences("ellipsoid/rot170 on a side stream, mode %d" % mode, on_side[1:], ans) == 0


NON_FINITE = {
    "nan_in_static_0": ("stat", 0, np.nan),
    "nan_in_static_700": ("stat", 700, np.nan),
    "inf_in_rest_3": ("rest", 3, np.inf),
}


TILE_RULE = ("a NaN coordinate in the FIRST target of a 512-target tile: genpc_chamfer_forward follows the reference's tile rule and "
             "answers (NaN 0x7fc00000, index 0) for all 1000 queries of direction 1; the seeded kernel's minimum over keys drops "
             "the NaN target and answers the nearest finite one, e.g. (0x38dddc18, 37) for query 0 -- 1000 of 1000 queries "
             "differ in both arithmetic modes and under every seeding; direction 2 agrees")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant", [pytest.param(v, marks=pytest.mark.xfail(strict=True, reason=TILE_RULE)) if v == "nan_in_static_0" else v
                                     for v in NON_FINITE])
def test_non_finite_points_as_the_brute_force_filter(gp, oracle, variant, mode):
    """A NaN or Inf coordinate: the brute-force filter implements the reference's 512-target tile rule (csrc/nn.h,
    nn_exhaustive), the seeded kernel takes a plain minimum over keys -- and mode 2 of the loop chooses between them by
    timing.  The two on the same posed cloud, under three seedings.  A NaN in static point 700 (inside a tile) and an Inf in
    rest point 3 give the same bytes; a NaN in static point 0 (the first target of tile 0) does not: TILE_RULE, expected to
    fail until the seeded path follows the tile rule or the loop stays on the filter for such clouds."""
    which, row, value = NON_FINITE[variant]
    rest, center, params, stat = (np.array(a) for a in C.case("ellipsoid", "loop"))
    (stat if which == "stat" else rest)[0, row, 1] = value
    case = (rest, center, params, stat)
    with arith(gp, mode):
        none = C.seeds("none", oracle, rest, stat, mode)
        posed = step(gp, case, *none)[0]
        assert np.isfinite(posed).all() == (which == "stat")
        bf = brute_force(gp, posed, stat)
        wrong = 0
        for policy in ("none", "random", "brute force's answers"):
            s1, s2 = (bf[1], bf[3]) if policy.startswith("brute") else C.seeds(policy, oracle, posed, stat, mode)
            out = step(gp, case, s1, s2)
            assert out[0].tobytes() == posed.tobytes()
            wrong += differences("%s mode %d seeds %s: seeded vs genpc_chamfer_forward" % (variant, mode, policy), out[1:], bf)
    assert wrong == 0
