"""Every case of tests/depth_prompt_ragged_cases.py can tell a wrong kernel from a right one: asserted here on the CPU statement
alone (tests/depth_prompt_ragged_ref.py and the restated summation order), for the committed seeds.  A case that violates a
condition FAILS; none is skipped or filtered."""
import ctypes

import numpy as np
import pytest

import depth_prompt_ragged_cases as C
import depth_prompt_ragged_ref as REF


@pytest.mark.parametrize("name", C.NAMES)
def test_the_case_meets_its_conditions(oracle, name):
    """The decision margin of every scan with a visible point (the designed tie of nothing_visible (a) is the one exception),
    the stated order within n 2^-53 of fsum on every row, and what the case is there for (depth_prompt_ragged_cases.conditions)."""
    got = C.conditions(oracle, name)
    for what, ok in got:
        print("%s: %s: %s" % (name, what, "holds" if ok else "VIOLATED"))
    assert got and all(ok for _, ok in got), [what for what, ok in got if not ok]


def test_the_case_table():
    """The sizes, offsets and settings each case exists for (they are the smallest at which its path exists: not to be shrunk)."""
    sizes = lambda name: tuple(len(p) for p in C.case(name).scans[0])
    assert sizes("chunk_edges") == (3, 1023, 1024, 1025, 2048, 7, 1027)
    c = C.case("chunk_edges")
    off = lambda order: tuple(int(v) for v in np.cumsum([0] + [len(c.scans[0][j]) for j in order]))
    assert off(c.orders[0]) == (0, 3, 1026, 2050, 3075, 5123, 5130, 6157)
    assert [len(c.scans[0][j]) for j in c.orders[1]] == [7, 3, 1023, 1024, 1025, 2048, 1027]
    assert all(a % 1024 != b % 1024 for a, b in zip(off(c.orders[0])[1:5], off(c.orders[1])[2:6]))    # every residue changes
    assert (c.res, c.variants, c.rescale, c.padding) == (32, ((1, 2),), True, 0.15)
    assert sizes("many_chunks") == (65 * 1024 + 3, 300)
    c = C.case("many_chunks")
    assert (c.res, c.variants, c.rescale, c.padding) == (8, ((1, 2),), True, 0.0)
    assert sizes("widest_stamp") == (40, 1500)
    c = C.case("widest_stamp")
    assert (c.res, c.variants) == (50, ((4, 8), (32, 1))) and c.res * c.res % 256 != 0
    assert all(ps * rate == 32 for ps, rate in c.variants)
    seen = np.nonzero(c.scans[3][1][1])[0]
    assert list(seen) == list(range(0, 1500, 50))                   # only every 50th point visible in the chosen row
    assert sizes("one_pixel") == (5, 260) and (C.case("one_pixel").res, C.case("one_pixel").variants) == (1, ((1, 1),))
    assert sizes("no_rescale") == (300, 1029)
    c = C.case("no_rescale")
    assert (c.res, c.variants, c.rescale) == (64, ((2, 3),), False)
    r = [np.linalg.norm(p, axis=1).max() for p in c.scans[0]]
    assert all(0.9 < x <= 1.0 + 1e-6 for x in r), r                 # radius 1.0, every point in front of a camera at 1.6
    full = sizes("full_table")
    assert len(full) == 256 and full[0] == 0 and full[255] == 0
    assert full[1:255] == tuple(C.FULL_TABLE_CYCLE[j % 10] for j in range(1, 255))
    c = C.case("full_table")
    assert (c.res, c.variants, c.rescale, c.padding) == (16, ((1, 2),), True, 0.15)
    assert sizes("nothing_visible") == (300, 300, 300)
    c = C.case("nothing_visible")
    assert (c.res, c.variants) == (32, ((2, 3),))
    m = c.scans[3]
    assert not m[0].any() and not m[1][0].any() and m[1][1].any() and m[2][0].any() and m[2][1].any()


def test_both_choices_occur(oracle):
    chosen = {name: {r["chosen"] for r in C.reference(oracle, name) if r is not None} for name in C.NAMES}
    assert set().union(*chosen.values()) == {0, 1}
    assert chosen["chunk_edges"] == {0, 1}


def test_the_stated_order_is_an_order_of_its_own(oracle):
    """Bit comparisons with sums_in_the_stated_order can tell orders apart only where the order shows: on at least one row of
    many_chunks and one of chunk_edges it differs from the plain ascending sum, and on chunk_edges also from the order with the
    chunk's partial taken as w0 + (w1 + (w2 + w3)) -- the step that needs a bit below 2^-45 to show (near_plane's docstring)."""
    for name in ("many_chunks", "chunk_edges"):
        c, n_diff = C.case(name), 0
        for j, r in enumerate(C.reference(oracle, name)):
            for row in range(2):
                s = C.sums_in_the_stated_order(r["depth_rows"][row], c.scans[3][j][row])
                a = C.ascending_sum(r["depth_rows"][row], c.scans[3][j][row])
                print("%s scan %d row %d: stated %s ascending %s" % (name, j, row, s.hex(), a.hex()))
                n_diff += s != a
        assert n_diff >= 1, name
    c, n_diff = C.case("chunk_edges"), 0
    for j, r in enumerate(C.reference(oracle, "chunk_edges")):
        for row in range(2):
            d, m = r["depth_rows"][row], c.scans[3][j][row]
            n_diff += C.sums_in_the_stated_order(d, m) != C.sums_in_the_stated_order(d, m, chunk_partial=lambda w: w[:, 0] + (w[:, 1] + (w[:, 2] + w[:, 3])))
    assert n_diff >= 1


def test_the_stated_order_on_hand_made_rows():
    """The restatement against sums small enough to do by hand: powers of two that round differently in different orders."""
    # the ulp of 2^60 is 2^8: a 2^7 added to it is a tie and rounds to the even 2^60; 2^8 survives
    d = np.zeros(2048, np.float32)
    d[1], d[2], d[3] = np.float32(2.0 ** 60), np.float32(2.0 ** 7), np.float32(2.0 ** 7)
    m = np.ones(2048, np.uint8)
    assert C.sums_in_the_stated_order(d, m) == 2.0 ** 60                    # one thread, ascending: each 2^7 is lost
    d[:] = 0
    d[3], d[2], d[1] = np.float32(2.0 ** 60), np.float32(2.0 ** 7), np.float32(2.0 ** 7)
    assert C.sums_in_the_stated_order(d, m) == 2.0 ** 60 + 2.0 ** 8         # ... and the other way round they add up first
    d[:] = 0
    d[0], d[4 * 1], d[4 * 33] = np.float32(2.0 ** 60), np.float32(2.0 ** 7), np.float32(2.0 ** 7)
    assert C.sums_in_the_stated_order(d, m) == 2.0 ** 60 + 2.0 ** 8         # lanes 1 and 33 meet at xor 32, lane 0 at xor 1
    d[:] = 0
    d[0], d[4 * 1], d[4 * 2] = np.float32(2.0 ** 60), np.float32(2.0 ** 7), np.float32(2.0 ** 7)
    assert C.sums_in_the_stated_order(d, m) == 2.0 ** 60                    # lane 2 meets lane 0 at xor 2, lane 1 at xor 1
    d[:] = 0
    d[0], d[256], d[512], d[768] = np.float32(2.0 ** 60), np.float32(2.0 ** 7), np.float32(2.0 ** 7), np.float32(2.0 ** 7)
    assert C.sums_in_the_stated_order(d, m) == 2.0 ** 60                    # ((w0 + w1) + w2) + w3: every 2^7 is lost
    assert C.sums_in_the_stated_order(d, m, chunk_partial=lambda w: w[:, 0] + (w[:, 1] + (w[:, 2] + w[:, 3]))) == 2.0 ** 60 + 2.0 ** 9
    m[0] = 0
    assert C.sums_in_the_stated_order(d, m) == 3 * 2.0 ** 7                 # an invisible point adds nothing
    d = np.zeros(65 * 1024 + 1, np.float32)
    d[0], d[64 * 1024], d[65 * 1024] = np.float32(2.0 ** 60), np.float32(2.0 ** 7), np.float32(2.0 ** 7)
    m = np.ones(len(d), np.uint8)
    # chunk 64 goes to lane 0 in its second pass (2^60 + 2^7 = 2^60), chunk 65 to lane 1, whose 2^7 the butterfly then loses too
    assert C.sums_in_the_stated_order(d, m) == 2.0 ** 60
    d[65 * 1024] = np.float32(2.0 ** 8)
    assert C.sums_in_the_stated_order(d, m) == 2.0 ** 60 + 2.0 ** 8         # (a wave that stopped after one pass would say 2^60)


def test_the_unrescaled_arm_rounds_once_however_it_is_written(oracle):
    """project_rescale's rescale == 0 arm, (o + 1) * 0.5 in two operations, cannot be told from one fused multiply-add
    o * 0.5 + 0.5: halving is exact, so both are the one rounding of (o + 1) / 2 (no float o brings o + 1 near the subnormals:
    next to -1 the sum is exact and a multiple of 2^-24).  So no_rescale cannot catch that rewrite, and need not; what it does
    catch is the arm not being taken.  Shown on the case's own NDC coordinates (to an ulp: 2 uv - 1) and on seeded ones down to
    2^-28, where the double below is exact before it is rounded."""
    c = C.case("no_rescale")
    ndc = [oracle.get_uvs(c.scans[2][j], C.focal(), c.scans[0][j], rescale=False)[0].reshape(-1) * np.float32(2) - np.float32(1) for j in range(2)]
    o = np.concatenate(ndc + [(np.random.default_rng(3).random(100000, dtype=np.float32) * 8 - 4), np.float32([-1, 1, 0, -3, 3, 2.0 ** -28, -1 + 2.0 ** -24])])
    o = o[np.abs(o) >= 2.0 ** -28]
    two = (o + np.float32(1.0)) * np.float32(0.5)
    fused = (o.astype(np.float64) * 0.5 + 0.5).astype(np.float32)
    assert two.dtype == np.float32 and np.array_equal(two.view(np.uint32), fused.view(np.uint32))
    # ... while the arm itself shows: with rescale on, the same scans give other pixels
    r = C.reference(oracle, "no_rescale")[0]
    on = oracle.get_uvs(c.scans[2][0], C.focal(), c.scans[0][0], rescale=True, padding=c.padding)[0][r["chosen"]]
    assert not np.array_equal(oracle.uv_to_pixels(on, c.res), r["pix"])


def test_the_table_at_its_limit_plans(oracle):
    """full_table through the host entry point: every empty scan refused by its number, the first of them scan 0."""
    from genpc_amd import build
    build.build(verbose=False)
    from genpc_amd import _lib
    c = C.case("full_table")
    sizes = [len(p) for p in c.scans[0]]
    off = (ctypes.c_int * 257)(*np.cumsum([0] + sizes).tolist())
    out = (ctypes.c_longlong * 7)()
    assert _lib.lib.genpc_depth_prompt_ragged_plan(256, ctypes.cast(off, ctypes.c_void_p), c.res, 1, 2, ctypes.cast(out, ctypes.c_void_p)) == 1, _lib.last_error()
    empties = sum(1 for n in sizes if n == 0)
    assert empties == 78 and out[3] == empties and out[4] == 0
    assert out[0] == (off[256] >> 10) + 256 and out[1] == 4 and out[2] == 1
    # the sample that is also run alone holds every size of the cycle and both neighbours of every kind of run of empty scans
    assert len(C.FULL_TABLE_SAMPLE) == 10 and {sizes[j] for j in C.FULL_TABLE_SAMPLE} == set(C.FULL_TABLE_CYCLE) - {0}
    for j in (2, 6, 8, 9, 12, 249, 252, 254):
        assert j in C.FULL_TABLE_SAMPLE and (j == 254 or sizes[j - 1] == 0 or sizes[j + 1] == 0)
    assert sizes[255] == 0 and sizes[1] == 0 and sizes[7] == 0 and sizes[10] == sizes[11] == 0 and sizes[250] == sizes[251] == 0


def test_nothing_visible_is_this_library_s_definition(oracle):
    """What a scan with points but no visible one gives (include/genpc_hip.h): the oracle's get_raw_depth cannot take an empty set
    (the reference's getDepth raises there), so images_ref states the paint of nothing itself; (b) goes to the row that sees."""
    c = C.case("nothing_visible")
    a, b, other = C.reference(oracle, "nothing_visible")
    with pytest.raises(ValueError):
        oracle.get_raw_depth(np.zeros((0, 2), np.int32), np.zeros(0, np.float32), np.zeros((0, 3), np.float32), c.res, 2, 3)
    assert a["sums"] == (0.0, 0.0) and a["chosen"] == 0 and not a["visible"].any()
    assert np.array_equal(a["images"], C.empty_images(c.res))
    assert (a["images"][:3] == 0).all() and (a["images"][3] == 1).all()
    # uv, depth and pix of the chosen row are stated as always
    uv2, d2, _, _ = oracle.get_uvs(c.scans[2][0], C.focal(), c.scans[0][0], rescale=True, padding=0.15)
    assert np.array_equal(a["uv"], uv2[0]) and np.array_equal(a["depth"], d2[0]) and np.array_equal(a["pix"], oracle.uv_to_pixels(uv2[0], c.res))
    # (b): every depth at these cameras is positive (znear 1e-2, zfar 1e2, the eye 1.6 from a ball of radius 0.5: the NDC depth
    # 1.0002 - 0.020002 / |z| with |z| in [1.1, 2.1] lies in [0.98, 0.991]), so the row that sees anything has the larger sum
    assert (b["depth_rows"] > 0.98).all() and (b["depth_rows"] < 0.991).all()
    assert b["sums"][0] == 0.0 and b["sums"][1] > 0 and b["chosen"] == 1 and b["visible"].any()
    assert other["visible"].any() and REF.margin_ok(other["sums"], 300)
