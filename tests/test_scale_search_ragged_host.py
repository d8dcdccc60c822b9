"""The host side of the ragged scale search, without a GPU: genpc_scale_search_scores_ragged and genpc_scale_search_ragged_plan
are declared, bound and exported and the ABI version stands; every refusal of the C entry points comes back as -1 with its
message before anything touches a device (null stream, dummy pointers: nothing is enqueued); the exported plan is the header's
at both sides of its boundary; and what reg_xyz.scale_search_scores_ragged and reg_xyz.iterative_scale_searches refuse."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_abi import header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = ctypes.c_void_p(0x1000)          # never dereferenced: every case below is decided on the host
NULL = ctypes.c_void_p(0)
PREFIX = "genpc_scale_search_scores_ragged: "


@pytest.fixture(scope="module")
def L():
    from genpc_amd import build
    build.build(verbose=False)
    from genpc_amd import _lib
    return _lib


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def cast(a):
    return NULL if a is None else ctypes.cast(a, ctypes.c_void_p)


def call(L, c, soff, toff, koff, ptr=DUMMY):
    return L.lib.genpc_scale_search_scores_ragged(c, cast(soff), cast(toff), cast(koff), ptr, ptr, ptr, 0.5, ptr, None)


def max_pairs():
    m = re.search(r"#define\s+GENPC_SCALE_SEARCH_RAGGED_MAX_PAIRS\s+(\d+)", open(os.path.join(ROOT, "include", "genpc_hip.h")).read())
    assert m, "the header exports the bound as a constant"
    return int(m.group(1))


def test_declared_bound_and_exported(L):
    p = header_prototypes()
    assert p.get("genpc_scale_search_scores_ragged") == 10      # c, 3 tables, 2 clouds, scales, weight, scores + stream
    assert p.get("genpc_scale_search_ragged_plan") == 3
    assert len(L.SIGNATURES["genpc_scale_search_scores_ragged"][1]) == 10
    assert len(L.SIGNATURES["genpc_scale_search_ragged_plan"][1]) == 3
    assert set(p) == set(L.SIGNATURES)
    assert L.lib.genpc_scale_search_scores_ragged is not None and L.lib.genpc_scale_search_ragged_plan is not None
    assert L.ABI_VERSION == 28 and L.lib.genpc_abi_version() == 28      # additive: the number stays
    from genpc_amd import reg_xyz
    assert max_pairs() == 256 and reg_xyz.SCALE_SEARCH_RAGGED_MAX_PAIRS == max_pairs()


def test_refusals(L):
    n = max_pairs()
    ok = ints(0, 5, 9)
    zeros = ints(*([0] * (n + 2)))
    cases = [
        ("negative number of pairs", -1, ints(0), ints(0), ints(0)),
        ("more than %d pairs" % n, n + 1, zeros, zeros, zeros),
        ("null offset table", 2, None, ok, ok),
        ("null offset table", 2, ok, None, ok),
        ("null offset table", 2, ok, ok, None),
        ("offsets must start at 0", 2, ints(1, 5, 9), ok, ok),
        ("offsets must start at 0", 2, ok, ints(1, 5, 9), ok),
        ("offsets must start at 0", 2, ok, ok, ints(1, 5, 9)),
        ("offsets must ascend", 2, ints(0, 9, 5), ok, ok),
        ("offsets must ascend", 2, ok, ints(0, 9, 5), ok),
        ("offsets must ascend", 2, ok, ok, ints(0, 9, 5)),
        ("more than 2^28 points", 2, ints(0, 1 << 28, (1 << 28) + 1), ok, ok),
        ("more than 2^28 points", 2, ok, ints(0, 1 << 28, (1 << 28) + 1), ok),
        ("more than 2^20 candidates", 2, ok, ok, ints(0, 1 << 20, (1 << 20) + 1)),
        ("pair 1 has candidates and an empty source", 2, ints(0, 5, 5), ok, ints(0, 1, 12)),
        ("pair 0 has candidates and an empty target", 2, ok, ints(0, 0, 9), ints(0, 1, 12)),
    ]
    for msg, c, soff, toff, koff in cases:
        assert call(L, c, soff, toff, koff) == -1, msg
        err = L.last_error()
        assert err.startswith(PREFIX) and msg in err, (msg, err)


def test_a_null_device_pointer_with_work_to_do_is_refused(L):
    assert call(L, 2, ints(0, 5, 9), ints(0, 5, 9), ints(0, 1, 3), ptr=NULL) == -1
    assert L.last_error() == PREFIX + "null pointer"


def test_nothing_to_do_returns_1(L):
    assert call(L, 0, None, None, None, ptr=NULL) == 1                                   # no pair: not even the tables are looked at
    assert call(L, 2, ints(0, 5, 9), ints(0, 0, 9), ints(0, 0, 0), ptr=NULL) == 1        # no candidate: empty clouds are legal then


def plan(L, c, soff):
    out = ints(-1, -1, -1)
    rc = L.lib.genpc_scale_search_ragged_plan(c, cast(soff), cast(out))
    return rc, tuple(out)


def boundary(L):
    """The largest source count of the one launch (the plan is monotone there: tests/scale_search_ragged_plan_check.cpp)."""
    lo, hi = 1, 1 << 20
    assert plan(L, 1, ints(0, lo))[1][:2] == (1, 0) and plan(L, 1, ints(0, hi))[1][:2] == (0, 1)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if plan(L, 1, ints(0, mid))[1][0] == 1 else (lo, mid - 1)
    return lo


def test_the_exported_plan(L):
    last = boundary(L)
    assert 2500 < last < 12000, last
    # csrc/scale_search_ragged_plan.h by hand: 192 fixed bytes, 16 a point, a table of cells + 1 ints rounded to 16 bytes;
    # 100 points get the ragged build's own budget of 100 + 64 cells
    lds100 = 192 + 16 * 100 + (100 + 64 + 1 + 3) // 4 * 16
    assert plan(L, 1, ints(0, 100)) == (1, (1, 0, lds100))
    rc, (fused, loop, lds_last) = plan(L, 1, ints(0, last))
    assert (rc, fused, loop) == (1, 1, 0) and lds100 < lds_last <= 160 * 1024 - 1024 and lds_last > 160 * 1024 - 1024 - 64
    assert plan(L, 1, ints(0, last + 1)) == (1, (0, 1, 0))
    assert plan(L, 0, None) == (1, (0, 0, 0))
    assert plan(L, 3, ints(0, 100, 100, 200)) == (1, (2, 0, lds100))                     # the pair without a source is on neither side
    assert plan(L, 3, ints(0, 100, 100 + last + 1, 100 + 2 * last + 1)) == (1, (2, 1, lds_last))
    assert L.lib.genpc_scale_search_ragged_plan(1, cast(ints(0, 5)), NULL) == -1
    for c, soff, msg in ((-1, ints(0), "negative number of pairs"), (2, None, "null offset table"), (2, ints(1, 2, 3), "offsets must start at 0"),
                         (2, ints(0, 3, 2), "offsets must ascend"), (max_pairs() + 1, ints(*([0] * (max_pairs() + 2))), "more than")):
        rc, out = plan(L, c, soff)
        assert rc == -1 and out == (0, 0, 0)
        err = L.last_error()
        assert err.startswith("genpc_scale_search_ragged_plan: ") and msg in err, err


def clouds(*sizes):
    return [torch.arange(n * 3, dtype=torch.float32).reshape(n, 3) for n in sizes]


def test_the_python_wrappers_refuse(L):
    from genpc_amd import reg_xyz
    f, one = reg_xyz.scale_search_scores_ragged, np.ones((2, 3))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        f(clouds(5, 7), clouds(6, 8), [one, one])
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        f((torch.zeros(12, 3), [0, 5, 12]), (torch.zeros(12, 3), [0, 6, 12]), [one, one])
    with pytest.raises(TypeError, match="float32"):
        f([c.double() for c in clouds(5)], clouds(6), [one])
    with pytest.raises(ValueError, match=r"targets\[0\] must be an \[N,3\] tensor"):
        f(clouds(5), [torch.zeros(6, 2)], [one])
    with pytest.raises(ValueError, match="2 sources against 1 targets"):
        f(clouds(5, 7), clouds(6), [one, one])
    with pytest.raises(ValueError, match="one .* per pair"):
        f(clouds(5, 7), clouds(6, 8), [one])
    with pytest.raises(ValueError, match="one .* per pair"):
        f(clouds(5, 7), clouds(6, 8), one)
    with pytest.raises(ValueError, match=r"scales\[1\] must be \[K,3\]"):
        f(clouds(5, 7), clouds(6, 8), [one, np.ones((2, 4))])
    with pytest.raises(ValueError, match="pair 1 has candidates and an empty target"):
        f(clouds(5, 7), clouds(6, 0), [one, one])
    with pytest.raises(ValueError, match="pair 0 has candidates and an empty source"):
        f(clouds(0, 7), clouds(6, 8), [one, one])
    assert f([], [], []) == []
    g, r3 = reg_xyz.iterative_scale_searches, [(0.8, 1.2)] * 3
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        g(clouds(5, 7), clouds(6, 8), r3, 3)
    with pytest.raises(ValueError, match="2 sources against 1 targets"):
        g(clouds(5, 7), clouds(6), r3, 3)
    with pytest.raises(TypeError, match="float32"):
        g(clouds(5), [c.double() for c in clouds(6)], r3, 3)
    with pytest.raises(ValueError, match=r"sources\[0\] must be an \[N,3\] tensor"):
        g([torch.zeros(5, 2)], clouds(6), r3, 3)
    with pytest.raises(ValueError, match="scale_ranges is three"):
        g(clouds(5, 7), clouds(6, 8), [(0.8, 1.2)] * 2, 3)
    with pytest.raises(ValueError, match="scale_ranges is three"):
        g(clouds(5, 7), clouds(6, 8), [r3], 3)
    with pytest.raises(ValueError, match="init_transforms is None or a list"):
        g(clouds(5, 7), clouds(6, 8), r3, 3, init_transforms=[np.eye(4)])
    with pytest.raises(ValueError, match=r"init_transforms\[1\] must be \[4,4\]"):
        g(clouds(5, 7), clouds(6, 8), r3, 3, init_transforms=[None, np.eye(3)])
    with pytest.raises(ValueError, match="pair 1 has candidates and an empty target"):
        g(clouds(5, 7), clouds(6, 0), r3, 3)
    assert g([], [], r3, 3) == []
