"""The plan of an all-pairs ragged nearest-neighbour call (csrc/nn_ragged_dense_plan.h) and the host side of its switch, without
a GPU: the header is plain C++ and is checked by a stand-alone program under the address and undefined-behaviour sanitizers
(tests/nn_ragged_dense_plan_check.cpp; nothing loaded into Python is sanitized); the exported plan and the per-thread mode touch
no GPU and are called here; the Python keywords refuse an unknown word before any library call and CPU tensors as ever."""
import ctypes
import os
import re
import shutil
import subprocess
import threading

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genpc_amd", "csrc")


def test_nn_ragged_dense_plan_program_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "nn_ragged_dense_plan_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", CSRC, os.path.join(ROOT, "tests", "nn_ragged_dense_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "nn_ragged_dense_plan_check: ok" in r.stdout, r.stdout


def test_nn_ragged_dense_plan_header_needs_no_hip():
    text = open(os.path.join(CSRC, "nn_ragged_dense_plan.h")).read()
    assert not re.search(r"#include\s*[<\"]hip|__device__|__global__|__shared__|hipStream_t", text)
    assert re.findall(r"#include\s*(\S+)", text) == ["<stddef.h>", '"ragged_table.h"']          # nothing else of the project


def test_the_kernel_file_and_its_neighbours():
    """One kernel in a file of its own; the launcher reads the plan; the grid call's two halves are untouched; the loop's step
    names the choice as a field of its plan."""
    dense = open(os.path.join(CSRC, "nn_ragged_dense.hip")).read()
    assert re.findall(r"__global__\s+(?:__launch_bounds__\([^)]*\)\s*)?void\s+(\w+)\s*\(", dense) == ["nn_ragged_dense_kernel"]
    assert "nn_ragged_dense_plan(t)" in dense and "workspace(" not in dense and "ws_alloc(" not in dense
    assert "s_sleep" not in dense and "atomic" not in dense.split("#include")[1]
    assert "int nn_ragged_dense(" in open(os.path.join(CSRC, "nn.h")).read()
    pose = open(os.path.join(CSRC, "pose.hip")).read()
    i = pose.index("static int pose_ragged_step(")
    step = pose[i:pose.index("\n}\n", i)]
    assert "plan.nn_dense" in step and step.count("nn_ragged_dense(") == 2
    assert pose.count("ask.nn_dense = t_nn_ragged_dense;") == 2


@pytest.fixture(scope="module")
def L():
    from genpc_amd import _lib
    return _lib


def _plan(L, noff, moff):
    na, ma = (ctypes.c_int * len(noff))(*noff), (ctypes.c_int * len(moff))(*moff)
    out = (ctypes.c_int * 8)()
    rc = L.lib.genpc_nn_ragged_dense_plan(len(noff) - 1, ctypes.cast(na, ctypes.c_void_p), ctypes.cast(ma, ctypes.c_void_p),
                                          ctypes.cast(out, ctypes.c_void_p))
    return rc, list(out)


def test_the_exported_plan(L):
    rc, out = _plan(L, [0, 65, 65, 300], [0, 7, 7, 2000])
    assert rc == 1
    items, threads, queries, tile, share, lds, lo, hi = out
    assert (threads, queries) == (256, 64) and tile == share * (threads // 64) and lds == tile * 16 + 16 and lds <= 64 * 1024
    assert items == (300 >> 6) + 3
    assert (hi << 32) | (lo & 0xffffffff) == 65 * 7 + 235 * 1993
    rc, out = _plan(L, [0], [0])                                   # no pair: the constants all the same
    assert rc == 1 and out[1:6] == [threads, queries, tile, share, lds] and out[0] == 0
    # the two refusals, by name; the 64-bit count is reported all the same
    h = (1 << 18) + 1
    rc, out = _plan(L, [0, h], [0, h])
    assert rc == -1 and "genpc_nn_ragged_dense_plan" in L.last_error() and "2^36" in L.last_error()
    assert (out[7] << 32) | (out[6] & 0xffffffff) == h * h
    rc, out = _plan(L, [0, 2], [0, (1 << 20) + 1])
    assert rc == -1 and "2^20" in L.last_error()
    assert _plan(L, [0, 2], [0, 1 << 20])[0] == 1
    assert _plan(L, [0, 1 << 18], [0, 1 << 18])[0] == 1
    # what the grid call refuses of a table
    assert _plan(L, [0, 5], [0, 0])[0] == -1 and "queries and no targets" in L.last_error()
    assert _plan(L, [0, 5, 3], [0, 1, 2])[0] == -1


def test_the_mode_is_per_thread_and_restored(L):
    lib = L.lib
    assert lib.genpc_nn_ragged_tune(0) == 0                        # the default is the grid search
    assert lib.genpc_nn_ragged_tune(2) == -1 and "genpc_nn_ragged_tune" in L.last_error()
    assert lib.genpc_nn_ragged_tune(-1) == -1
    assert lib.genpc_nn_ragged_tune(0) == 0                        # ... and a refused value left it
    with L.nn_ragged_search("dense"):
        seen = []
        t = threading.Thread(target=lambda: seen.append(lib.genpc_nn_ragged_tune(0)))
        t.start()
        t.join()
        assert seen == [0]                                         # a second host thread starts in grid mode
        with L.nn_ragged_search(None):                             # None leaves the mode alone
            assert lib.genpc_nn_ragged_tune(1) == 1
        with L.nn_ragged_search("grid"):
            assert lib.genpc_nn_ragged_tune(0) == 0
        assert lib.genpc_nn_ragged_tune(1) == 1                    # restored behind the inner block
    assert lib.genpc_nn_ragged_tune(0) == 0
    with pytest.raises(KeyError):
        with L.nn_ragged_search("dense"):
            raise KeyError("inside")
    assert lib.genpc_nn_ragged_tune(0) == 0                        # restored on an exception too
    # not part of the exported thread state: the eight ints are what they were
    before = L.thread_state()
    with L.nn_ragged_search("dense"):
        assert L.thread_state() == before


def test_python_keywords_refuse_before_any_library_call(L, monkeypatch):
    import torch
    from genpc_amd import chamfer_3D, reg_xyz
    from genpc_amd.loss_functions.Chamfer3D.dist_chamfer_ragged import chamfer_ragged
    from genpc_amd.optim_registration import diff_obj_pose

    calls = []

    class Recorder:
        def __getattr__(self, name):
            def f(*a):
                calls.append(name)
                return 1
            return f
    for mod in (chamfer_3D, diff_obj_pose, reg_xyz):
        monkeypatch.setattr(mod, "_L", Recorder())
    monkeypatch.setattr(L, "lib", Recorder())
    x = torch.zeros(4, 3)
    d, i = torch.zeros(4), torch.zeros(4, dtype=torch.int32)
    for bad in ("Dense", "brute", 1, "", b"dense"):
        with pytest.raises(ValueError, match='"grid" or "dense"'):
            chamfer_3D.nm_distance_ragged(x, [0, 4], x, [0, 4], d, i, search=bad)
        with pytest.raises(ValueError, match='"grid" or "dense"'):
            chamfer_ragged([x], [x], search=bad)
        with pytest.raises(ValueError, match='nn_search must be None, "grid" or "dense"'):
            diff_obj_pose.object_pose_optimization_scans([x], [x], nn_search=bad)
        with pytest.raises(ValueError, match='nn_search must be None, "grid" or "dense"'):
            diff_obj_pose.pose_loss_grad_ragged([x], torch.zeros(1, 3), torch.zeros(1, 10), [x], 0.02, nn_search=bad)
        with pytest.raises(ValueError, match='nn_search must be None, "grid" or "dense"'):
            reg_xyz.reg_tensors_scans([x], [x], ragged_pose=True, nn_search=bad)
    # CPU tensors are refused as today, whatever the keyword says
    for ok in (None, "grid", "dense"):
        with pytest.raises(RuntimeError, match="GPU tensors only"):
            chamfer_3D.nm_distance_ragged(x, [0, 4], x, [0, 4], d, i, search=ok)
        with pytest.raises(RuntimeError, match="GPU tensors only"):
            chamfer_ragged([x], [x], search=ok)
        with pytest.raises(RuntimeError, match="GPU tensors only"):
            diff_obj_pose.object_pose_optimization_scans([x], [x], nn_search=ok)
        with pytest.raises(RuntimeError, match="GPU tensors only"):
            diff_obj_pose.pose_loss_grad_ragged([x], torch.zeros(1, 3), torch.zeros(1, 10), [x], 0.02, nn_search=ok)
        with pytest.raises(RuntimeError, match="GPU tensors only"):
            reg_xyz.reg_tensors_scans([x], [x], ragged_pose=True, nn_search=ok)
    assert calls == []
