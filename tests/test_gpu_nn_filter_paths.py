"""The f16 filter stages a full resident slice without a duplicate mask in a straight line, works out max |t'|^2 and the
non-finite flag in query block 0 alone, addresses its loads and stores from per-block scalar bases, and publishes its lists
with the two lane halves sharing the query tiles (csrc/nn_f16.hip).  None of that may change a result: every distance and every
index of both directions, bit for bit, against the oracle, at the smallest shapes that reach each path.  Which shape reaches
which form depends on the device's CU count: the shapes come from genpc_nn_plan (tests/nn_forms.py), and each case asserts
what the plan says of it -- the form, and whether every slice fills the LDS tile -- before it runs.

The share of exhaustively re-done queries (genpc_nn_stats, hook 512) is compared with the counts the commit before this
change gave on the same seeded input on an MI355X (256 CUs), PARENT_REDO: a changed slice maximum or list record shows there
first, long before a result is wrong."""
import ctypes

import numpy as np
import pytest

import nn_forms
from conftest import gen_pair

pytestmark = pytest.mark.gpu

F16 = 3
HOOK_STATS = 512
MODE = 1
WIDE_TILE = 2048          # targets per LDS tile of the wide and the 2048-tile forms; the other forms' is 1024

# (queries, exhaustive re-dos) of one forward call at hook 512, from the commit before this change on an MI355X
PARENT_REDO = {
    ((1, 6144, 3), (1, 32768, 3)): (38912, 0),
    ((1, 16001, 3), (1, 16001, 3)): (32002, 0),
}
# Both of those are zero re-dos: equality there only shows that none were added.  The three calls of the triplicated input of
# case (e) on the first shape above gave these counts before the change; the first call's is far from both ends, so a slice
# maximum or a list record that moved either way shows in it.
PARENT_REDO_TRIPLICATES = {
    ((1, 6144, 3), (1, 32768, 3)): [(38912, 38783), (38912, 0), (38912, 0)],
}


@pytest.fixture(scope="module")
def gp():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib, chamfer_3D
    from genpc_amd.loss_functions import chamfer_3DDist
    return dict(torch=torch, lib=_lib.lib, cd=chamfer_3DDist(), fwd=chamfer_3D.forward)


def plan_of(gp, shape):
    return nn_forms.plan(gp["lib"], F16, shape[0][0], shape[0][1], shape[1][1])


def all_full(p, shape, tile):
    """Every slice of both directions fills the LDS tile: the straight-line path in every block (no mask given)."""
    return p["slice_len"] == tile and shape[0][1] % tile == 0 and shape[1][1] % tile == 0


_found = {}


def cheapest_full(gp, says, tile, batches=(1,), step=None):
    """The cheapest shape, by b n m, with both sizes multiples of `step` (default: the tile) whose plan `says` and whose slices
    all fill the tile; None where there is none up to 32768 points."""
    key = (says.__name__, tile, batches, step)
    if key not in _found:
        step = step or tile
        best = None
        for b in batches:
            for n in range(step, 32768 + 1, step):
                for m in range(step, 32768 + 1, step):
                    if best is not None and b * n * m >= best[0]:
                        break
                    shape = ((b, n, 3), (b, m, 3))
                    p = plan_of(gp, shape)
                    if not p["too_large"] and says(p) and all_full(p, shape, tile):
                        best = (b * n * m, shape)
        _found[key] = best[1] if best else None
    return _found[key]


def is_wide(p):
    return p["q"] == 4 and p["form"] == nn_forms.WIDE


def is_four_wave_1024(p):
    return p["q"] == 4 and p["form"] == nn_forms.FOUR_WAVE


def is_q2(p):
    return p["q"] == 2


def need(gp, shape, what):
    """A searched shape, or the assertion that this device is none of those the search is known to succeed on."""
    if shape is None:
        cus = nn_forms.plan(gp["lib"], F16, 1, 37, 37)["cus"]
        assert cus != 256, "no shape reaches %s on %d CUs" % (what, cus)
        pytest.skip("no shape of the search space reaches %s on %d CUs" % (what, cus))
    return shape


def run_f16(gp, a, b, hooks=0, calls=1):
    """`calls` forward calls (synchronised, as separate steps of a loop are) with the f16 family forced; the last one's outputs and
    every call's (queries, re-dos) where hook 512 counts them."""
    torch, lib = gp["torch"], gp["lib"]
    prev_mode = lib.genpc_set_arith(MODE)
    prev_path = lib.genpc_nn_tune(F16, hooks)
    buf = (ctypes.c_ulonglong * 3)()
    counts = []
    try:
        A, B = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        for _ in range(calls):
            if hooks & HOOK_STATS:
                lib.genpc_nn_stats(ctypes.cast(buf, ctypes.c_void_p), 1, None)
            out = gp["cd"](A, B)
            torch.cuda.synchronize()
            if hooks & HOOK_STATS:
                lib.genpc_nn_stats(ctypes.cast(buf, ctypes.c_void_p), 1, None)
                counts.append((int(buf[0]), int(buf[1])))
    finally:
        lib.genpc_set_arith(prev_mode)
        lib.genpc_nn_tune(prev_path, 0)
    return [t.cpu().numpy() for t in out], counts


def assert_bits(got, exp, msg):
    """Bit for bit -- except that a NaN distance need only be a NaN (its sign and payload are not defined by IEEE 754 and differ
    between the oracle's host and the GPU; tests/test_gpu_nn_prologue_loads.py sets the same bar)."""
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
        if variant == "triplicates":
            # every slice of 2048 targets holds its first 682 points three times, 683 apart: three bookkeeping units of one list
            # with the same minimum for nearly every query -- the exhaustive pass, until the duplicate pre-pass masks the copies
            for c in (a, b):
                for s in range(0, c.shape[1], WIDE_TILE):
                    c[:, s + 683:s + 683 + 682] = c[:, s:s + 682]
                    c[:, s + 1366:s + 1366 + 682] = c[:, s:s + 682]
        elif variant == "non_finite":
            # one NaN and one inf coordinate, in slices 1 and 2 of each cloud (different axes in the two clouds, so that no
            # inf - inf appears: its NaN has no defined sign, and this test compares bits)
            a[0, WIDE_TILE + 5, 0] = np.nan
            a[0, 2 * WIDE_TILE + 77, 0] = np.inf
            b[0, WIDE_TILE + 9, 1] = np.nan
            b[0, 2 * WIDE_TILE + 131, 1] = np.inf
        for c in (a, b):
            c.setflags(write=False)
        _inputs[key] = (a, b)
    return _inputs[key]


_expected = {}


def expected(oracle, shape, variant):
    key = (shape, variant)
    if key not in _expected:
        a, b = pair(shape, variant)
        _expected[key] = [np.array(x) for x in oracle.chamfer_forward(np.array(a), np.array(b), MODE)]
    return _expected[key]


def check(gp, oracle, shape, variant="plain", hooks=0, calls=1):
    p = plan_of(gp, shape)
    assert p["family"] == F16 and not p["too_large"], (shape, p)
    a, b = pair(shape, variant)
    got, counts = run_f16(gp, np.array(a), np.array(b), hooks, calls)
    assert_bits(got, expected(oracle, shape, variant), "%s %s hooks %d: %s" % (shape, variant, hooks, nn_forms.describe(p)))
    return counts


def assert_parent_share(gp, shape, counts):
    cus = plan_of(gp, shape)["cus"]
    if shape not in PARENT_REDO:
        assert cus != 256, "no count of the commit before the change recorded for %s" % (shape,)
        return
    assert counts[-1] == PARENT_REDO[shape], "queries and exhaustive re-dos %s, before the change %s" % (counts[-1], PARENT_REDO[shape])


def test_wide_every_slice_full(gp, oracle):
    """(a) The straight-line path in every block: the wide form, clouds that are multiples of its 2048-target slices and of its
    1024-query blocks."""
    shape = need(gp, cheapest_full(gp, is_wide, WIDE_TILE), "the wide form with full slices")
    p = plan_of(gp, shape)
    assert is_wide(p) and all_full(p, shape, WIDE_TILE) and shape[0][1] % 1024 == 0 and shape[1][1] % 1024 == 0, (shape, p)
    counts = check(gp, oracle, shape, hooks=HOOK_STATS)
    assert_parent_share(gp, shape, counts)


def test_wide_partial_last_slice_and_last_block(gp, oracle):
    """(b) Both paths in one launch: seven full slices and a partial one per direction, a last query block that is partly empty and
    a last 32-query tile that holds one query.  That the shape is wide with slices of 2048 is asserted on 256 CUs, the MI355X;
    elsewhere the case runs whatever form the plan gives it and proves nothing about which paths it reached."""
    shape = ((1, 16001, 3), (1, 16001, 3))
    p = plan_of(gp, shape)
    if p["cus"] == 256:
        assert is_wide(p) and p["slice_len"] == WIDE_TILE and p["slices0"] == 8, p
    assert 16001 % WIDE_TILE and 16001 % 1024 and 16001 % 32 == 1
    counts = check(gp, oracle, shape, hooks=HOOK_STATS)
    assert_parent_share(gp, shape, counts)


@pytest.mark.parametrize("form", ["f16_q4_tile2048", "f16_q4_four_wave", "f16_q4_three_wave", "f16_q2"])
def test_other_forms_still_answer(gp, oracle, form):
    """(c) The instances that share the template, each at the cheapest shape the plan sends there (no size a multiple of 32:
    partial slices, the general path)."""
    found = nn_forms.cheapest(gp["lib"], form)
    shape = need(gp, found and ((found[0], found[1], 3), (found[0], found[2], 3)), form)
    assert nn_forms.FORMS[form][1](plan_of(gp, shape)), (form, shape)
    check(gp, oracle, shape)


@pytest.mark.parametrize("says", [is_four_wave_1024, is_q2], ids=["q4_four_wave", "q2"])
def test_1024_tile_forms_full_slices(gp, oracle, says):
    """(c) The straight-line path in the 1024-target-tile forms: 512-query blocks of four waves, and the 256-query blocks, whose
    lane halves publish one query tile each."""
    shape = need(gp, cheapest_full(gp, says, 1024, batches=(1, 2, 3, 4)), "a 1024-tile form with full slices")
    p = plan_of(gp, shape)
    assert says(p) and all_full(p, shape, 1024), (shape, p)
    check(gp, oracle, shape)


def test_directions_on_different_paths(gp, oracle):
    """(d) N != M: direction 0's targets fill every slice, direction 1's leave a partial last one -- and its queries a partial
    last tile -- in the same launch.  As in (b), which form and paths the shape reaches is asserted on 256 CUs only."""
    shape = ((1, 16001, 3), (1, 16384, 3))
    p = plan_of(gp, shape)
    if p["cus"] == 256:
        assert is_wide(p) and p["slice_len"] == WIDE_TILE, p
    check(gp, oracle, shape)


def test_duplicates_switch_the_pre_pass_on(gp, oracle):
    """(e) Targets with exact triplicates, three calls: the first finds the pre-pass off and re-does more than a 32nd of its
    queries, which switches the pre-pass on for the calls behind it (csrc/chamfer.hip: the policy's own threshold); with the
    mask present every block takes the general path, the copies are staged as padding, and the re-dos fall below the threshold
    again.  All three calls' results are the oracle's, and on the device the counts were recorded on they are the counts of the
    commit before this change, the first call's 38783 of 38912 among them."""
    torch = gp["torch"]
    shape = need(gp, cheapest_full(gp, is_wide, WIDE_TILE), "the wide form with full slices")
    clean = torch.rand(1, 4096, 3, device="cuda")
    for _ in range(3):              # whatever came before, the policy's switch is off again
        gp["cd"](clean, clean.flip(1).contiguous())
        torch.cuda.synchronize()
    counts = check(gp, oracle, shape, "triplicates", hooks=HOOK_STATS, calls=3)
    (q0, r0), (q2, r2) = counts[0], counts[-1]
    assert q0 == q2 == shape[0][0] * (shape[0][1] + shape[1][1]), counts
    assert r0 * 32 > q0, "the first call should have asked for the pre-pass: %s" % (counts,)
    assert r2 * 32 < q2, "the pre-pass should have been on for the last call: %s" % (counts,)
    if shape in PARENT_REDO_TRIPLICATES:
        assert counts == PARENT_REDO_TRIPLICATES[shape], "queries and exhaustive re-dos %s, before the change %s" % (counts, PARENT_REDO_TRIPLICATES[shape])
    else:
        assert plan_of(gp, shape)["cus"] != 256, "no counts of the commit before the change recorded for %s" % (shape,)


def test_non_finite_targets_in_later_slices(gp, oracle):
    """(f) A NaN and an inf coordinate in slices 1 and 2: the flag that makes the finish step answer the cloud's queries with the
    reference's 512-target-tile semantics is now raised by query block 0 alone."""
    shape = need(gp, cheapest_full(gp, is_wide, WIDE_TILE), "the wide form with full slices")
    assert min(shape[0][1], shape[1][1]) >= 3 * WIDE_TILE
    check(gp, oracle, shape, "non_finite")


def test_batch_of_two(gp, oracle):
    """(g) The batch offset in the scalar bases: B = 2 at the smallest wide shape whose slices are all full."""
    shape = need(gp, cheapest_full(gp, is_wide, WIDE_TILE, batches=(2,)), "the wide form with full slices at B = 2")
    p = plan_of(gp, shape)
    assert shape[0][0] == 2 and is_wide(p) and all_full(p, shape, WIDE_TILE), (shape, p)
    check(gp, oracle, shape)
