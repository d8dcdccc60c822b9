"""The f16 filter and its finish step request their prologue loads back to back (queries, resident slice, duplicate
mask words; list words, slice maxima, query, centre; the best unit's pieces ahead of the fp64 threshold).  Nothing of
that may change a result: every distance and every index of both directions, bit for bit, against the oracle, at the
smallest shapes that reach the reordered lines -- clamped lanes and tails, the wide single-round form, the multi-round
forms, the duplicate pre-pass forced on, and non-finite coordinates."""
import numpy as np
import pytest

from conftest import gen_pair

pytestmark = pytest.mark.gpu

F16 = 3
HOOK_DEDUPE_ON = 4096

# Q = 2 forms: clamped lanes (fewer queries than a tile), tails of every kind, fewer than 16 targets
SMALL = [((1, 1, 3), (1, 1, 3)), ((1, 31, 3), (1, 33, 3)), ((1, 33, 3), (1, 2049, 3)), ((2, 127, 3), (2, 513, 3)),
         ((3, 1000, 3), (3, 37, 3))]
# Q = 4, one round, 8-wave blocks; no size a multiple of 32, 1024 or 2048
WIDE = ((1, 10501, 3), (1, 10007, 3))
# several rounds: three waves per SIMD, and 2048-target LDS tiles with 4 waves
ROUNDS = [((3, 9001, 3), (3, 12003, 3)), ((4, 4099, 3), (4, 8209, 3))]


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


def check(gp, oracle, shape, variant, mode, hooks=0):
    a, b = pair(shape, variant)
    got = run_f16(gp, np.array(a), np.array(b), mode, hooks)
    assert_bits(got, expected(oracle, shape, variant, mode), "%s %s mode %d hooks %d" % (shape, variant, mode, hooks))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "%dx%d_vs_%d" % (s[0][0], s[0][1], s[1][1]))
def test_clamped_lanes_and_tails(gp, oracle, shape, mode):
    check(gp, oracle, shape, "plain", mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_wide_single_round_form(gp, oracle, mode):
    check(gp, oracle, WIDE, "plain", mode)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", ROUNDS, ids=lambda s: "%dx%d_vs_%d" % (s[0][0], s[0][1], s[1][1]))
def test_multi_round_forms(gp, oracle, shape, mode):
    check(gp, oracle, shape, "plain", mode)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", [WIDE, ROUNDS[1]], ids=["wide", "rounds"])
def test_duplicate_pre_pass_forced(gp, oracle, shape, mode):
    """Mask words loaded first, bits taken afterwards -- including the word of target nt - 1, which clamped lanes read."""
    exp = expected(oracle, shape, "dup", mode)
    # the first copy of each pair answers: no index points into the last 100 targets (the later copies) of either cloud,
    # although queries sit exactly on them
    n, m = shape[0][1], shape[1][1]
    assert (exp[2] < m - 100).all() and (exp[3] < n - 100).all()
    check(gp, oracle, shape, "dup", mode, HOOK_DEDUPE_ON)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("variant", ["nan_first", "inf_first"])
def test_non_finite_coordinates(gp, oracle, variant, mode):
    """A query at infinity (it must not set the block's scale), slice maxima of +inf, and the exhaustive pass behind the
    reordered loads.  nan_first: the NaN sits at index 0, the head of the reference's first tile, so every query of that
    direction ends with (NaN, 0); inf_first: it sits at the end, and ordinary answers remain."""
    check(gp, oracle, WIDE, variant, mode)
