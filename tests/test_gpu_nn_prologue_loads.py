"""The f16 filter and its finish step request their prologue loads back to back (queries, resident slice, duplicate
mask words; list words, slice maxima, query, centre; the best unit's pieces ahead of the fp64 threshold).  Nothing of
that may change a result: every distance and every index of both directions, bit for bit, against the oracle, at the
smallest shapes that reach the reordered lines -- clamped lanes and tails, the wide single-round form, the multi-round
forms, the duplicate pre-pass forced on, and non-finite coordinates.  Which shape reaches which form depends on the device's CU
count: the shapes of the named forms come from genpc_nn_plan (tests/nn_forms.py), and each test asserts what the plan says
before it runs; the literal shapes below stay as further cases whatever they reach here."""
import numpy as np
import pytest

import nn_forms
from conftest import gen_pair

pytestmark = pytest.mark.gpu

F16 = 3
HOOK_DEDUPE_ON = 4096

# Q = 2 forms: clamped lanes (fewer queries than a tile), tails of every kind, fewer than 16 targets
SMALL = [((1, 1, 3), (1, 1, 3)), ((1, 31, 3), (1, 33, 3)), ((1, 33, 3), (1, 2049, 3)), ((2, 127, 3), (2, 513, 3)),
         ((3, 1000, 3), (3, 37, 3))]
# Q = 4 (2e8 pairs and more); no size a multiple of 32, 1024 or 2048.  On 64 CUs: one round, 8-wave blocks ...
WIDE = ((1, 10501, 3), (1, 10007, 3))
# ... three waves per SIMD, and 2048-target LDS tiles with 4 waves; on 256 CUs the first takes four-wave blocks with slices of
# 896 targets and these two are wide.  What they reach on the device at hand is in each failure's message.
ROUNDS = [((3, 9001, 3), (3, 12003, 3)), ((4, 4099, 3), (4, 8209, 3))]
# the forms the tests are named after, each at the cheapest shape of tests/nn_forms.py's search space that reaches it here
SEARCHED = {"wide": "f16_q4_wide", "three_wave": "f16_q4_three_wave", "tile2048": "f16_q4_tile2048"}


@pytest.fixture(scope="module")
def gp():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib
    from genpc_amd.loss_functions import chamfer_3DDist
    return dict(torch=torch, lib=_lib.lib, cd=chamfer_3DDist())


def run_f16(gp, a, b, mode, hooks=0):
    torch, lib = gp["torch"], gp["lib"]
    prev_mode = lib.genpc_set_arith(mode)
    prev_path = lib.genpc_nn_tune(F16, hooks)
    try:
        out = gp["cd"](torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
        torch.cuda.synchronize()
    finally:
        lib.genpc_set_arith(prev_mode)
        lib.genpc_nn_tune(prev_path, 0)
    return [t.cpu().numpy() for t in out]


def assert_bits(got, exp, msg):
    """Bit for bit -- except that a NaN distance need only be a NaN: the sign and payload of a NaN that arithmetic
    on a NaN coordinate returns are not defined by IEEE 754 and differ between the oracle's host and the GPU (the query
    that carries the NaN coordinate itself: 1 of 10501 distances; tests/test_gpu_chamfer_parity.py sets the same bar)."""
    for g, e, nme in zip(got, exp, ("dist1", "dist2", "idx1", "idx2")):
        g, e = np.ascontiguousarray(g), np.ascontiguousarray(e)
        assert g.shape == e.shape, (nme, msg, g.shape, e.shape)
        gb, eb = g.view(np.uint32).ravel(), e.view(np.uint32).ravel()
        differ = gb != eb
        if g.dtype == np.float32:
            differ &= ~(np.isnan(g.ravel()) & np.isnan(e.ravel()))
        bad = np.flatnonzero(differ)
        assert bad.size == 0, "%s %s: %d of %d differ, first at %d: got %r (0x%08x), expected %r (0x%08x)" % (
            nme, msg, bad.size, g.size, bad[0], g.ravel()[bad[0]], gb[bad[0]], e.ravel()[bad[0]], eb[bad[0]])


_inputs = {}


def pair(shape, variant="plain"):
    """Inputs of a case, made once and never written to afterwards."""
    key = (shape, variant)
    if key not in _inputs:
        a, b = gen_pair(sum(shape[0]) + sum(shape[1]), *shape)
        if variant == "dup":
            # the last 100 points of each cloud over the 100 before them: later copies up to the last mask word
            for c in (a, b):
                c[:, -200:-100] = c[:, -100:]
        elif variant in ("nan_first", "inf_first"):
            # one NaN and one inf coordinate at the two ends of each cloud (different axes in the two clouds, so that
            # no inf - inf appears: its NaN has no defined sign, and this test compares bits)
            lo, hi = (np.nan, np.inf) if variant == "nan_first" else (np.inf, np.nan)
            a[0, 0, 0] = lo
            a[0, -1, 0] = hi
            b[0, 0, 1] = lo
            b[0, -1, 1] = hi
        for c in (a, b):
            c.setflags(write=False)
        _inputs[key] = (a, b)
    return _inputs[key]


_expected = {}


def expected(oracle, shape, variant, mode):
    key = (shape, variant, mode)
    if key not in _expected:
        a, b = pair(shape, variant)
        _expected[key] = [np.array(x) for x in oracle.chamfer_forward(np.array(a), np.array(b), mode)]
    return _expected[key]


def searched(gp, form):
    """The shape that reaches `form` (a key of SEARCHED) on this device, or None where the search space holds none -- which is
    the case at none of 256, 64 and 32 CUs."""
    found = nn_forms.cheapest(gp["lib"], SEARCHED[form])
    if found is None:
        cus = nn_forms.plan(gp["lib"], F16, 1, 37, 37)["cus"]
        assert cus not in (256, 64, 32), "no shape reaches %s on %d CUs" % (form, cus)
        return None
    b, n, m = found
    return ((b, n, 3), (b, m, 3))


def check(gp, oracle, shape, variant, mode, hooks=0, form=None):
    """Runs the f16 family at `shape` after asserting what genpc_nn_plan says of it: the f16 filter, and `form` (a key of
    SEARCHED) where one is claimed."""
    p = nn_forms.plan(gp["lib"], F16, shape[0][0], shape[0][1], shape[1][1])
    assert p["family"] == F16 and not p["too_large"], (shape, p)
    if form is not None:
        assert nn_forms.FORMS[SEARCHED[form]][1](p), (form, shape, p)
    a, b = pair(shape, variant)
    got = run_f16(gp, np.array(a), np.array(b), mode, hooks)
    assert_bits(got, expected(oracle, shape, variant, mode), "%s %s mode %d hooks %d: %s" % (shape, variant, mode, hooks, nn_forms.describe(p)))


def check_form_and_literal(gp, oracle, form, literal, variant, mode, hooks=0):
    """The searched shape of `form`, asserted to reach it, then the literal shape that carried the name before."""
    shape = searched(gp, form)
    if shape is not None:
        check(gp, oracle, shape, variant, mode, hooks, form)
    p = nn_forms.plan(gp["lib"], F16, literal[0][0], literal[0][1], literal[1][1])
    assert p["q"] == 4, (literal, p)
    check(gp, oracle, literal, variant, mode, hooks)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "%dx%d_vs_%d" % (s[0][0], s[0][1], s[1][1]))
def test_clamped_lanes_and_tails(gp, oracle, shape, mode):
    check(gp, oracle, shape, "plain", mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_wide_single_round_form(gp, oracle, mode):
    check_form_and_literal(gp, oracle, "wide", WIDE, "plain", mode)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", ROUNDS, ids=lambda s: "%dx%d_vs_%d" % (s[0][0], s[0][1], s[1][1]))
def test_multi_round_forms(gp, oracle, shape, mode):
    check(gp, oracle, shape, "plain", mode)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("form", ["three_wave", "tile2048"])
def test_multi_round_forms_by_plan(gp, oracle, form, mode):
    """Three waves per SIMD, and 2048-target LDS tiles with 4 waves, at shapes the plan sends there on this device."""
    shape = searched(gp, form)
    if shape is None:
        pytest.skip("no shape of the search space reaches %s on this device" % form)
    check(gp, oracle, shape, "plain", mode, form=form)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", [("wide", WIDE), ("tile2048", ROUNDS[1])], ids=["wide", "rounds"])
def test_duplicate_pre_pass_forced(gp, oracle, shape, mode):
    """Mask words loaded first, bits taken afterwards -- including the word of target nt - 1, which clamped lanes read."""
    form, literal = shape
    for s in (searched(gp, form), literal):
        if s is None:
            continue
        exp = expected(oracle, s, "dup", mode)
        # the first copy of each pair answers: no index points into the last 100 targets (the later copies) of either cloud,
        # although queries sit exactly on them
        n, m = s[0][1], s[1][1]
        assert (exp[2] < m - 100).all() and (exp[3] < n - 100).all()
        check(gp, oracle, s, "dup", mode, HOOK_DEDUPE_ON, form if s is not literal else None)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("variant", ["nan_first", "inf_first"])
def test_non_finite_coordinates(gp, oracle, variant, mode):
    """A query at infinity (it must not set the block's scale), slice maxima of +inf, and the exhaustive pass behind the
    reordered loads.  nan_first: the NaN sits at index 0, the head of the reference's first tile, so every query of that
    direction ends with (NaN, 0); inf_first: it sits at the end, and ordinary answers remain."""
    check_form_and_literal(gp, oracle, "wide", WIDE, variant, mode)
