"""The device-side check of a farthest point sampling (csrc/fps_verify.hip: fps_verify_kernel and the poisoning kernel behind it,
through genpc_fps_verify_probe) against the definition (oracle.fps_check): every right sequence of tests/fps_check_cases.py
passes, every mutant -- wrong in one step and nowhere else -- fails, for every number of segments and in both arithmetic
modes.  A verdict is a bit: out[0] stays 0 or becomes -2; there is no tolerance.  What a case is, is decided on the CPU
(tests/test_fps_check_definition.py)."""
import ctypes
import time

import numpy as np
import pytest

import fps_check_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fg():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib
    clouds = {name: torch.from_numpy(x.copy()).cuda() for name, x in C.clouds().items()}
    return dict(torch=torch, lib=_lib, L=_lib.lib, clouds=clouds)


class Packed:
    """The cases' sequences and minima side by side in two device arrays, and the probe's host tables for calls of eight."""

    def __init__(self, fg, groups):
        torch = fg["torch"]
        self.groups = groups
        flat = [c for g in groups for c in g]
        off = np.concatenate([[0], np.cumsum([c["k"] for c in flat])]).astype(np.int64)
        self.first = torch.from_numpy(off[:-1].copy()).cuda()
        self.idx0 = torch.from_numpy(np.concatenate([c["idx"] for c in flat]).astype(np.int32)).cuda()
        self.idx = self.idx0.clone()
        self.minima = torch.from_numpy(np.concatenate([c["minima"] for c in flat]).astype(np.float32)).cuda()
        self.expect = np.array([0 if c["expect"] == -1 else -2 for c in flat], np.int32)
        self.flat = flat
        self.calls = []
        q = 0
        for g in groups:
            nj = len(g)
            xs = [fg["clouds"][c["cloud"]] for c in g]
            self.calls.append((nj, (ctypes.c_int * nj)(*[int(x.shape[0]) for x in xs]), (ctypes.c_int * nj)(*[c["k"] for c in g]),
                               (ctypes.c_void_p * nj)(*[x.data_ptr() for x in xs]),
                               (ctypes.c_void_p * nj)(*[self.idx.data_ptr() + 4 * int(off[q + s]) for s in range(nj)]),
                               (ctypes.c_void_p * nj)(*[self.minima.data_ptr() + 4 * int(off[q + s]) for s in range(nj)])))
            q += nj

    def verdicts(self, fg, mode, nseg, single):
        """One probe call per group on fresh copies of the sequences -> out[0] of every case."""
        L = fg["L"]
        self.idx.copy_(self.idx0)
        prev = L.genpc_set_arith(mode)
        try:
            for nj, n, k, x, o, p in self.calls:
                rc = fg["lib"].on_device_of(self.idx, L.genpc_fps_verify_probe, nj, ctypes.addressof(n), ctypes.addressof(k),
                                            ctypes.addressof(x), ctypes.addressof(o), ctypes.addressof(p), nseg, single)
                assert rc == 1, fg["lib"].last_error()
        finally:
            L.genpc_set_arith(prev)
        got = self.idx[self.first].cpu().numpy()
        # (the check writes nothing but the verdict)
        rest = self.idx.clone()
        rest[self.first] = self.idx0[self.first]
        assert fg["torch"].equal(rest, self.idx0)
        return got

    def mismatches(self, got):
        return [(c["cloud"], "kind %d" % c["kind"], "step %d" % c["j"], sorted(c["cls"]), "want %d got %d" % (e, g))
                for c, e, g in zip(self.flat, self.expect, got) if e != g]


_packed = {}


def packed_cases(fg, mode):
    """All cases of a mode in calls of eight, in a fixed shuffled order: right and wrong, small and large clouds side by side."""
    if mode not in _packed:
        cases = C.cases(mode)
        order = np.random.default_rng(8).permutation(len(cases))
        groups = [[cases[i] for i in order[g:g + 8]] for g in range(0, len(cases), 8)]
        _packed[mode] = Packed(fg, groups)
    return _packed[mode]


@pytest.mark.parametrize("single", [0, 1])
@pytest.mark.parametrize("nseg", C.NSEGS)
@pytest.mark.parametrize("mode", [0, 1])
def test_check_verdicts_are_the_definitions(fg, mode, nseg, single):
    """Every case: the probe's verdict is the reference's -- 0 where oracle.fps_check returned -1, -2 otherwise."""
    P = packed_cases(fg, mode)
    t0 = time.perf_counter()
    got = P.verdicts(fg, mode, nseg, single)
    dt = time.perf_counter() - t0
    right = sum(1 for c in P.flat if c["kind"] == 0)
    print("mode %d nseg %d single %d: %d right sequences, %d mutants, %d calls, %.0f ms"
          % (mode, nseg, single, right, len(P.flat) - right, len(P.calls), dt * 1e3))
    bad = P.mismatches(got)
    assert not bad, (len(bad), bad[:20])


@pytest.mark.parametrize("mode", [0, 1])
def test_check_job_tables_poison_the_wrong_cloud_alone(fg, mode):
    """Eight clouds of different n and k in one call, cut into 1 and 3 segments (a cloud's rows of segment minima lie behind the
    earlier clouds'): all right, then the mutant in slot q = 0 .. 7 -- the verdict is bad for cloud q alone."""
    P = Packed(fg, C.tables(mode))
    for nseg in C.TABLE_NSEG:
        got = P.verdicts(fg, mode, nseg, 0).reshape(9, 8)
        want = np.zeros((9, 8), np.int32)
        want[np.arange(1, 9), np.arange(8)] = -2
        assert np.array_equal(P.expect.reshape(9, 8), want)
        np.testing.assert_array_equal(got, want, err_msg="nseg %d" % nseg)


def test_a_timed_out_sampling_keeps_its_mark(fg):
    """out[0] == -1 (the sampler gave up) fails the check and stays -1: the caller tells the two apart."""
    right = [c for c in C.cases(1) if c["kind"] == 0 and c["cloud"] == "uniform129" and c["k"] == 129]
    c = dict(right[0])
    c["idx"] = c["idx"].copy()
    c["idx"][0] = -1
    c["expect"] = 0
    P = Packed(fg, [[c, right[0]]])
    for nseg in (0, 2):
        assert P.verdicts(fg, 1, nseg, 0).tolist() == [-1, 0]


def test_probe_refusals(fg):
    torch = fg["torch"]
    L = fg["L"]
    x = fg["clouds"]["uniform9"]
    idx = torch.zeros(9, dtype=torch.int32, device="cuda")
    pd = torch.zeros(9, dtype=torch.float32, device="cuda")

    def call(nj=1, n=9, k=9, xs=None, os_=None, ps=None, nseg=0, tables=(True, True, True, True, True)):
        m = max(nj, 1)
        arr = [(ctypes.c_int * m)(*([n] * m)), (ctypes.c_int * m)(*([k] * m)),
               (ctypes.c_void_p * m)(*([x.data_ptr() if xs is None else xs] * m)),
               (ctypes.c_void_p * m)(*([idx.data_ptr() if os_ is None else os_] * m)),
               (ctypes.c_void_p * m)(*([pd.data_ptr() if ps is None else ps] * m))]
        args = [ctypes.addressof(a) if t else None for a, t in zip(arr, tables)]
        return fg["lib"].on_device_of(x, L.genpc_fps_verify_probe, nj, *args, nseg, 0)

    refused = [dict(nj=0), dict(nj=9), dict(k=0), dict(k=10), dict(nseg=-1), dict(nseg=17), dict(xs=0), dict(os_=0), dict(ps=0)]
    refused += [dict(tables=tuple(t != s for t in range(5))) for s in range(5)]
    for kw in refused:
        assert call(**kw) == -1 and b"genpc_fps_verify_probe" in L.genpc_last_error(), kw
    torch.cuda.synchronize()
    assert int(idx.abs().sum()) == 0          # (a refused call touches nothing)
    assert call(nseg=16) == 1                 # (all-zero minima of a zero sequence: wrong, and poisoned)
    assert int(idx[0]) == -2
