"""The four kernels that take NNArgs read their arguments in one round at entry, select the direction's fields from both
directions' values and decode (query block, batch element, slice) / (batch element, finish block) by multiplying
(csrc/nn.h NN_ARG, csrc/nn_decode.h).  Nothing of that may change a result: every distance and every index, bit for bit,
against the oracle, at shapes where a wrong decode or a field of the wrong direction shows -- b in {1, 3, 7}, clouds of
different sizes (direction 1's fields differ from direction 0's), several query blocks and several slices in counts that are
no powers of two -- through each family (VALU, fp32 MFMA, f16), both arithmetic modes, both directions in one call and one
direction alone (genpc_nm_distance); the wide and the 2048-target-tile forms of the f16 filter at the cheapest b = 1 shape
with unequal clouds that tests/nn_forms.py finds for the device at hand; the duplicate mask on; and hooks 8 and 16, which are
arguments that now load at entry."""
import numpy as np
import pytest

import nn_forms
from conftest import gen_pair

pytestmark = pytest.mark.gpu

VALU, MFMA32, F16 = nn_forms.VALU, nn_forms.MFMA32, nn_forms.F16
HOOK_ALL_EXHAUSTIVE, HOOK_ALL_LISTED, HOOK_DEDUPE_ON = 8, 16, 4096

# (b, n, m).  700 x 1300: two or three query blocks against three to six; 1300 x 37: a direction with ONE slice of 37 targets beside one
# of several; 3001 x 5003: MANY, below
SHAPES = [(1, 700, 1300), (3, 700, 1300), (7, 700, 1300), (1, 1300, 37), (7, 1300, 37), (3, 3001, 5003)]
FAMILIES = {"valu": VALU, "mfma32": MFMA32, "f16": F16}
MANY = (3, 3001, 5003)      # the shape that stands for "several query blocks and several slices, in counts that are no powers of two"


def no_power_of_two(v):
    return v >= 3 and v & (v - 1) != 0


def says_many(p):
    """What MANY must be on the device at hand, asserted before it runs (a change of the plan must not quietly make it a trivial
    decode).  The query blocks depend on the family alone: 6 and 10 (VALU), 24 and 40 (fp32 MFMA), 12 and 20 (f16).  The slices
    depend on the CU count: from 128 CUs on every family gives both directions several (at 256: 20 and 12, 8 and 5, 10 and 6) and at
    least one count that is no power of two; a smaller device may give the fp32 family one or two, which is not asserted there."""
    ok = no_power_of_two(p["qblocks0"]) and (p["slices1"] == 0 or no_power_of_two(p["qblocks1"]))
    if p["cus"] >= 128:
        ok = ok and p["slices0"] > 1 and (p["slices1"] == 0 or (p["slices1"] > 1 and (no_power_of_two(p["slices0"]) or no_power_of_two(p["slices1"]))))
    return ok


@pytest.fixture(scope="module")
def gp():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib, chamfer_3D
    return dict(torch=torch, lib=_lib.lib, fwd=chamfer_3D.forward, nm=chamfer_3D.nm_distance)


_inputs, _expected = {}, {}


def pair(shape, variant="plain"):
    """Inputs of a case, made once and never written to afterwards."""
    key = (shape, variant)
    if key not in _inputs:
        b, n, m = shape
        a, c = gen_pair(b + n + m, (b, n, 3), (b, m, 3))
        if variant == "dup":
            # the last 100 points of each cloud over the 100 before them: later copies up to the last mask word
            for x in (a, c):
                x[:, -200:-100] = x[:, -100:]
        for x in (a, c):
            x.setflags(write=False)
        _inputs[key] = (a, c)
    return _inputs[key]


def expected(oracle, shape, variant, mode):
    key = (shape, variant, mode)
    if key not in _expected:
        a, c = pair(shape, variant)
        _expected[key] = [np.array(x) for x in oracle.chamfer_forward(np.array(a), np.array(c), mode)]      # d1, d2, i1, i2
    return _expected[key]


def run(gp, shape, variant, family, mode, hooks=0, one_direction=False):
    torch, lib = gp["torch"], gp["lib"]
    b, n, m = shape
    a, c = (torch.from_numpy(np.array(x)).cuda() for x in pair(shape, variant))
    d1 = torch.full((b, n), -1.0, device="cuda")
    d2 = torch.full((b, m), -1.0, device="cuda")
    i1 = torch.full((b, n), -7, device="cuda", dtype=torch.int32)
    i2 = torch.full((b, m), -7, device="cuda", dtype=torch.int32)
    # (genpc_nn_tune returns the previous family only, and hooks once set cannot be unset: a case without hooks leaves the
    # thread's hooks as they are (-1); a case with hooks ends with 0, the value of a thread on which none was ever set unless
    # GENPC_NN_DEBUG is, which no test of this suite sets)
    prev_mode = lib.genpc_set_arith(mode)
    prev_path = lib.genpc_nn_tune(family, hooks if hooks else -1)
    try:
        if one_direction:
            gp["nm"](a, c, d1, i1)
        else:
            gp["fwd"](a, c, d1, d2, i1, i2)
        torch.cuda.synchronize()
    finally:
        lib.genpc_set_arith(prev_mode)
        lib.genpc_nn_tune(prev_path, 0 if hooks else -1)
    return [t.cpu().numpy() for t in ((d1, i1) if one_direction else (d1, d2, i1, i2))]


def assert_bits(got, exp, names, msg):
    for g, e, nme in zip(got, exp, names):
        g, e = np.ascontiguousarray(g), np.ascontiguousarray(e)
        assert g.shape == e.shape, (nme, msg, g.shape, e.shape)
        gb, eb = g.view(np.uint32).ravel(), e.view(np.uint32).ravel()
        bad = np.flatnonzero(gb != eb)
        assert bad.size == 0, "%s %s: %d of %d differ, first at %d: got %r (0x%08x), expected %r (0x%08x)" % (
            nme, msg, bad.size, g.size, bad[0], g.ravel()[bad[0]], gb[bad[0]], e.ravel()[bad[0]], eb[bad[0]])


def check(gp, oracle, shape, family, mode, variant="plain", hooks=0, says=None):
    b, n, m = shape
    p = nn_forms.plan(gp["lib"], family, b, n, m)
    assert not p["too_large"] and (says is None or says(p)), (shape, p)
    exp = expected(oracle, shape, variant, mode)
    msg = "%s %s mode %d hooks %d: %s" % (shape, variant, mode, hooks, nn_forms.describe(p))
    assert_bits(run(gp, shape, variant, family, mode, hooks), exp, ("dist1", "dist2", "idx1", "idx2"), msg)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_vs_%d" % s)
def test_both_directions(gp, oracle, shape, family, mode):
    check(gp, oracle, shape, FAMILIES[family], mode, says=says_many if shape == MANY else None)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_vs_%d" % s)
def test_one_direction(gp, oracle, shape, family, mode):
    """genpc_nm_distance: ndir = 1, the second direction's arguments are zeros."""
    b, n, m = shape
    p = nn_forms.plan(gp["lib"], FAMILIES[family], b, n, m, ndir=1)
    assert shape != MANY or says_many(p), (shape, p)
    exp = expected(oracle, shape, "plain", mode)
    got = run(gp, shape, "plain", FAMILIES[family], mode, one_direction=True)
    assert_bits(got, (exp[0], exp[2]), ("dist", "idx"), "%s mode %d one direction: %s" % (shape, mode, nn_forms.describe(p)))


def searched(gp, name):
    """The cheapest shape of tests/nn_forms.py's search space with b = 1 and unequal clouds whose plan on this device is of
    form `name`; None where there is none (at 256, 64 and 32 CUs there is one for both forms)."""
    family, says = nn_forms.FORMS[name]
    lib = gp["lib"]
    shapes = sorted((n * m, n, m) for n in nn_forms.SIZES for m in nn_forms.SIZES if n != m and n * m <= nn_forms.PAIR_LIMIT)
    for _, n, m in shapes:
        p = nn_forms.plan(lib, family, 1, n, m)
        if says(p) and not p["too_large"]:
            return (1, n, m)
    cus = nn_forms.plan(lib, F16, 1, 37, 37)["cus"]
    assert cus not in (256, 64, 32), "no b = 1 shape with unequal clouds reaches %s on %d CUs" % (name, cus)
    return None


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["f16_q4_wide", "f16_q4_tile2048"])
def test_f16_forms_of_512_query_blocks(gp, oracle, name, mode):
    shape = searched(gp, name)
    if shape is None:
        pytest.skip("no b = 1 shape of the search space reaches %s on this device" % name)
    check(gp, oracle, shape, F16, mode, says=nn_forms.FORMS[name][1])


@pytest.mark.parametrize("mode", [0, 1])
def test_duplicate_mask_on(gp, oracle, mode):
    """A cloud with repeated points, the pre-pass forced: dupmask and dup_shared of the block's direction."""
    shape = MANY
    exp = expected(oracle, shape, "dup", mode)
    assert (exp[2] < shape[2] - 100).all() and (exp[3] < shape[1] - 100).all()      # the first copy of each pair answers
    check(gp, oracle, shape, F16, mode, "dup", HOOK_DEDUPE_ON)


@pytest.mark.parametrize("hook", [HOOK_ALL_EXHAUSTIVE, HOOK_ALL_LISTED])
def test_hooks_that_load_at_entry(gp, oracle, hook):
    """Hook 8: every query of the filtered paths is answered by the exhaustive pass; hook 16: every listed tile is evaluated.
    Both are read from the arguments at entry and used late; the results are the oracle's either way."""
    for family in (F16, MFMA32):
        check(gp, oracle, (3, 700, 1300), family, 1, hooks=hook)
