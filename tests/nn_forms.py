"""Which shapes reach which kernel form of the nearest-neighbour call, asked of the library (genpc_nn_plan, csrc/nn_plan.h) for the
device at hand -- the form a shape runs depends on the CU count, so no test assumes it.  Shared by tests/test_gpu_nn_forms.py,
tests/test_gpu_nn_prologue_loads.py and tests/test_gpu_chamfer_parity.py."""
import ctypes

VALU, MFMA32, F16 = 0, 1, 3
FOUR_WAVE, THREE_WAVE, TILE2048, WIDE = 0, 1, 2, 3
FORM_NAMES = {FOUR_WAVE: "four waves", THREE_WAVE: "three waves per SIMD", TILE2048: "four waves, 2048-target tile", WIDE: "eight waves (wide)"}
FIELDS = ("family", "form", "q", "unit", "nl", "slice_len", "slices0", "slices1", "blocks", "fin_blocks", "early", "too_large", "qblocks0", "qblocks1",
          "hint_stride", "cus")

# the search space: b <= 16, n and m from sizes that are no multiple of 32
SIZES = (37, 127, 257, 513, 1031, 1543, 2049, 3001, 4099, 5003, 6007, 7001, 8209, 9001, 10007, 12003, 14001, 16001, 16381, 20011, 24593, 28001, 32771)
BATCHES = tuple(range(1, 17))
PAIR_LIMIT = 7e8

# what to reach: (family to force, what the plan must say)
FORMS = {
    "f16_q2": (F16, lambda p: p["q"] == 2),
    "f16_q4_four_wave": (F16, lambda p: p["q"] == 4 and p["form"] == FOUR_WAVE),
    "f16_q4_three_wave": (F16, lambda p: p["q"] == 4 and p["form"] == THREE_WAVE),
    "f16_q4_tile2048": (F16, lambda p: p["q"] == 4 and p["form"] == TILE2048),
    "f16_q4_wide": (F16, lambda p: p["q"] == 4 and p["form"] == WIDE),
    "f16_nl1": (F16, lambda p: p["nl"] == 1),
    "f16_nl2": (F16, lambda p: p["nl"] == 2),
    "f16_unit2": (F16, lambda p: p["unit"] == 2),
    "f16_unit4": (F16, lambda p: p["unit"] == 4),
    "mfma32_u1": (MFMA32, lambda p: p["unit"] == 1),
    "mfma32_u2": (MFMA32, lambda p: p["unit"] == 2),
    "valu_r2": (VALU, lambda p: p["q"] == 2),
    "valu_r4": (VALU, lambda p: p["q"] == 4),
}


def plan(lib, family, b, n, m, ndir=2, cus=0):
    """The plan of a genpc_chamfer_forward (ndir 2) / genpc_nm_distance (ndir 1) call with `family` forced on the calling thread
    (None: as the thread stands); cus 0: the current device's."""
    out = (ctypes.c_int * 16)()
    prev = lib.genpc_nn_tune(-1 if family is None else family, -1)
    try:
        assert lib.genpc_nn_plan(int(b), int(n), int(m), ndir, cus, ctypes.cast(out, ctypes.c_void_p)) == 1
    finally:
        if family is not None:
            lib.genpc_nn_tune(prev, -1)
    p = dict(zip(FIELDS, out))
    assert family is None or p["family"] == family, (family, p)
    return p


_plans = {}


def _sweep(lib, family, cus):
    """Every shape of the search space with its plan, cheapest (b n m) first."""
    key = (family, cus)
    if key not in _plans:
        shapes = sorted((b * n * m, b, n, m) for b in BATCHES for n in SIZES for m in SIZES if b * n * m <= PAIR_LIMIT)
        _plans[key] = [(b, n, m, plan(lib, family, b, n, m, 2, cus)) for _, b, n, m in shapes]
    return _plans[key]


def cheapest(lib, name, cus=0):
    """(b, n, m) of the cheapest shape, by b n m, whose plan on `cus` CUs (0: the device's) is of form `name`; None if the search
    space holds none at or below PAIR_LIMIT pairs."""
    family, says = FORMS[name]
    for b, n, m, p in _sweep(lib, family, cus):
        if says(p) and not p["too_large"]:
            return b, n, m
    return None


def describe(p):
    """One phrase for a docstring or a message: what a plan runs."""
    if p["family"] == F16:
        return "f16 filter, Q = %d, %s, slices of %d (%d + %d), %d + %d blocks" % (
            p["q"], FORM_NAMES[p["form"]], p["slice_len"], p["slices0"], p["slices1"], p["blocks"], p["fin_blocks"])
    return {VALU: "VALU, R = %d" % p["q"], MFMA32: "fp32 MFMA, Q = %d, U = %d" % (p["q"], p["unit"])}.get(p["family"], "cell search")
