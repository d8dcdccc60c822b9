"""The hand-off of the f16 filter's candidate lists to the finish step: one 16-byte record per (list, query) at
[slice * NL + n][batch * nq + j] (csrc/nn.h ListRec, list_rec), stored by nn_f16_kernel with one 16-byte store per list and loaded
by nn_finish_kernel with one 16-byte load.  The f16 family is forced (genpc_nn_tune(3, 0)) and every distance and index of both
directions is compared with the oracle bit for bit, in both arithmetic modes.  The shapes are chosen for the record addressing and
the wide form's unit loop, not for size:
    1 x 37 x 37            one partial record row, NL = 2
    2 x 1000 x 517         batch offset, nq no multiple of 64 in either direction, unequal clouds
    3 x 2049 x 4099        several slices, one target past a tile
    wide                   the cheapest shape that reaches the eight-wave form on this device (tests/nn_forms.py)
    wide, one fewer each   the same without its last query and last target: odd tails
    wide, non-finite       the same with a NaN and a +inf coordinate in each cloud: the exhaustive path behind lists that are still
                           written and read
(On the CPU the oracle answers each of these in under half a second.)"""
import numpy as np
import pytest

import nn_forms
from conftest import gen_pair
from test_gpu_nn_prologue_loads import assert_bits

pytestmark = pytest.mark.gpu

CASES = ("1x37x37", "2x1000x517", "3x2049x4099", "wide", "wide_less_one", "wide_nonfinite")


@pytest.fixture(scope="module")
def gp():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib
    from genpc_amd.loss_functions import chamfer_3DDist
    return dict(torch=torch, lib=_lib.lib, cd=chamfer_3DDist())


_inputs, _expected = {}, {}


def inputs(gp, name):
    """(x, y, wide) of a case, made once and never written to afterwards"""
    if name not in _inputs:
        wide = name.startswith("wide")
        if wide:
            shape = nn_forms.cheapest(gp["lib"], "f16_q4_wide")
            assert shape is not None, "no shape of the search space reaches the wide form on this device"
        else:
            shape = tuple(int(v) for v in name.split("x"))
        b, n, m = shape
        x, y = gen_pair(b + n + m, (b, n, 3), (b, m, 3))
        if name == "wide_less_one":
            x, y = np.ascontiguousarray(x[:, :-1]), np.ascontiguousarray(y[:, :-1])
        if name == "wide_nonfinite":
            x[0, n // 3, 0] = np.nan
            x[b - 1, n - 2, 1] = np.inf
            y[0, m // 2, 1] = np.nan
            y[b - 1, 5, 2] = np.inf
        for c in (x, y):
            c.setflags(write=False)
        _inputs[name] = (x, y, wide)
    return _inputs[name]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", CASES)
def test_list_records_against_the_oracle(gp, oracle, name, mode):
    torch, lib = gp["torch"], gp["lib"]
    x, y, wide = inputs(gp, name)
    b, n, m = x.shape[0], x.shape[1], y.shape[1]
    if (name, mode) not in _expected:
        _expected[(name, mode)] = [np.array(v) for v in oracle.chamfer_forward(np.array(x), np.array(y), mode)]
    prev_mode = lib.genpc_set_arith(mode)
    prev_family = lib.genpc_nn_tune(nn_forms.F16, 0)
    try:
        p = nn_forms.plan(lib, None, b, n, m)          # as this thread stands: what the call below gets
        assert p["family"] == nn_forms.F16 and not p["too_large"], (name, (b, n, m), p)
        assert not wide or (p["q"] == 4 and p["form"] == nn_forms.WIDE), (name, (b, n, m), p)
        if name == "1x37x37":
            assert p["nl"] == 2, p
        got = gp["cd"](torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(y)).cuda())
        torch.cuda.synchronize()
    finally:
        lib.genpc_set_arith(prev_mode)
        lib.genpc_nn_tune(prev_family, 0)
    assert_bits([t.cpu().numpy() for t in got], _expected[(name, mode)], "%s %s mode %d: %s" % (name, (b, n, m), mode, nn_forms.describe(p)))
