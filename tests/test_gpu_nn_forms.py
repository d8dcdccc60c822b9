"""Every kernel form a nearest-neighbour call can take, on the device at hand: the f16 filter with Q = 2, the four forms of its
512-query blocks (four waves, three waves per SIMD, four waves with the 2048-target tile, eight-wave wide blocks), both list
counts per lane, both bookkeeping units, the fp32 MFMA family with U = 1 and 2, the VALU family with R = 2 and 4.  Which shape
reaches which form depends on the CU count, so each case asks genpc_nn_plan (csrc/nn_plan.h) for the cheapest shape of a fixed
search space (tests/nn_forms.py) that reaches its form here, asserts that the plan says so, and compares every distance and index
of both directions with the oracle, bit for bit, in both arithmetic modes."""
import numpy as np
import pytest

import nn_forms
from conftest import gen_pair
from test_gpu_nn_prologue_loads import assert_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gp():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib
    from genpc_amd.loss_functions import chamfer_3DDist
    return dict(torch=torch, lib=_lib.lib, cd=chamfer_3DDist())


_cases = {}


def case(gp, name):
    """(shape, inputs) of a form on this device, made once and never written to afterwards; None if no shape reaches it."""
    if name not in _cases:
        shape = nn_forms.cheapest(gp["lib"], name)
        if shape is None:
            _cases[name] = None
        else:
            b, n, m = shape
            x, y = gen_pair(b + n + m, (b, n, 3), (b, m, 3))
            for c in (x, y):
                c.setflags(write=False)
            _cases[name] = (shape, x, y)
    return _cases[name]


_expected = {}


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(nn_forms.FORMS))
def test_form_against_the_oracle(gp, oracle, name, mode):
    torch, lib = gp["torch"], gp["lib"]
    found = case(gp, name)
    family, says = nn_forms.FORMS[name]
    if found is None:
        # (at 256, 64 and 32 CUs every form has a shape: tests/test_nn_plan.py's table and the search space were checked there)
        cus = nn_forms.plan(lib, family, 1, 37, 37)["cus"]
        assert cus not in (256, 64, 32), "no shape reaches %s on %d CUs" % (name, cus)
        pytest.skip("no shape of the search space at or below %g pairs reaches %s on %d CUs" % (nn_forms.PAIR_LIMIT, name, cus))
    (b, n, m), x, y = found
    if (name, mode) not in _expected:
        _expected[(name, mode)] = [np.array(v) for v in oracle.chamfer_forward(np.array(x), np.array(y), mode)]
    prev_mode = lib.genpc_set_arith(mode)
    prev_family = lib.genpc_nn_tune(family, 0)
    try:
        p = nn_forms.plan(lib, None, b, n, m)          # as this thread stands: what the call below gets
        assert p["family"] == family and says(p) and not p["too_large"], (name, (b, n, m), p)
        got = gp["cd"](torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(y)).cuda())
        torch.cuda.synchronize()
    finally:
        lib.genpc_set_arith(prev_mode)
        lib.genpc_nn_tune(prev_family, 0)
    assert_bits([t.cpu().numpy() for t in got], _expected[(name, mode)], "%s %s mode %d: %s" % (name, (b, n, m), mode, nn_forms.describe(p)))
