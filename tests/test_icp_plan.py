"""Which implementation an ICP call runs (csrc/icp_plan.h): the one-workgroup solve with one of four cell budgets, or the
multi-launch loop, from the target count alone.  No GPU: the header is plain C++ and is checked by a stand-alone program under
the address and undefined-behaviour sanitizers (monotone in nt, inside a compute unit's LDS, the boundaries the layout gives by
hand, nothing fused from 65536 targets on); that genpc_icp_batch and the kernel decide nothing besides is checked as text, and
the exported genpc_icp_plan -- what tests/test_gpu_icp_paths.py takes its sizes from -- is the same function."""
import ctypes
import os
import re
import shutil
import subprocess

from test_pose_plan import _body

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genpc_amd", "csrc")


def test_icp_plan_program_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "icp_plan_check")
    # (the sanitizers' runtimes linked statically, as in tests/test_pose_plan.py)
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", CSRC, os.path.join(ROOT, "tests", "icp_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0 and "icp_plan_check: ok" in r.stdout, r.stdout


def test_icp_plan_header_needs_no_hip():
    text = open(os.path.join(CSRC, "icp_plan.h")).read()
    assert not re.search(r"#include\s*[<\"]hip|__device__|__global__|#include\s*\"(common|nn|grid)\.h\"", text)
    assert re.findall(r"#include\s*(\S+)", text) == ["<stddef.h>"]


def test_the_call_and_the_kernel_read_the_plan():
    """genpc_icp_batch takes its path, cell budget and LDS size from icp_plan(nt) and holds no LDS arithmetic of its own; the
    constants of the kernel's LDS layout are defined in icp_plan.h alone."""
    icp = open(os.path.join(CSRC, "icp.hip")).read()
    call = _body(icp, "GENPC_API int genpc_icp_batch(")
    code = "\n".join(l.split("//")[0] for l in call.splitlines())
    assert "icp_plan(nt)" in code
    assert re.search(r"if\s*\(\s*plan\.one_workgroup\s*\)", code)
    for word in ("icp_fused_lds", "kFFixed", "kFLds", "kFCells", "kFIndexLimit", "cells >>", "65536", "8192", "4096", "2048", "160"):
        assert word not in code, word
    assert not re.search(r"\b1024\b", code)
    # what is launched is what the plan says
    assert len(re.findall(r"dim3\(kFT\), lds, st", code)) == 2 and len(re.findall(r"\bplan\.cells\b", code)) == 2
    assert re.search(r"lds\s*=\s*\(size_t\)\s*plan\.lds_bytes", code)
    for name in ("kFT", "kFWaves", "kFItems", "kFFixed"):
        assert not re.search(r"constexpr\s+\w+\s+%s\b" % name, icp), name
        assert re.search(r"constexpr\s+\w+\s+%s\b" % name, open(os.path.join(CSRC, "icp_plan.h")).read()), name
    exported = _body(icp, "GENPC_API int genpc_icp_plan(")
    assert "genpc::icp_plan(nt)" in exported


def test_exported_plan_is_the_header_s():
    """genpc_icp_plan through ctypes (no GPU is touched) at each budget's last target count and the first multi-launch one."""
    from genpc_amd import _lib

    def plan(nt):
        out = (ctypes.c_int * 3)(-1, -1, -1)
        assert _lib.lib.genpc_icp_plan(nt, ctypes.cast(out, ctypes.c_void_p)) == 1
        return tuple(out)

    assert [plan(nt)[:2] for nt in (1, 4388, 4389, 5412, 5413, 5924, 5925, 6180, 6181, 65536)] == \
        [(1, 8192), (1, 8192), (1, 4096), (1, 4096), (1, 2048), (1, 2048), (1, 1024), (1, 1024), (0, 0), (0, 0)]
    assert plan(6180)[2] == 98880 + 4096 + 59784 and plan(6181)[2] == 0
    assert _lib.lib.genpc_icp_plan(100, None) == -1
