"""The launch plan of the ragged auction's bid kernel (csrc/emd_ragged_plan.h), without a GPU: the header is plain C++ and is
checked by a stand-alone program under the address and undefined-behaviour sanitizers (tests/emd_ragged_plan_check.cpp;
nothing loaded into Python is sanitized); that the kernels use it is checked as text."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genpc_amd", "csrc")


def test_emd_ragged_plan_program_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "emd_ragged_plan_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", CSRC, os.path.join(ROOT, "tests", "emd_ragged_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "emd_ragged_plan_check: ok" in r.stdout, r.stdout


def test_emd_ragged_plan_header_needs_no_hip():
    text = open(os.path.join(CSRC, "emd_ragged_plan.h")).read()
    assert not re.search(r"#include\s*[<\"]hip|__global__|#include\s*\"common.h\"", text)
    assert re.findall(r"#include\s*(\S+)", text) == ['"ragged_offsets.h"']          # (plain C++ itself: tests/test_ragged_offsets.py)


def test_the_kernels_take_their_pair_from_the_plan():
    """emd_ragged.hip plans once per call with the device's CU count, launches the bid kernel on the plan's grid, and every
    kernel finds its pair through the header's two lookups; scratch comes from the named slot through a WsLayout."""
    text = open(os.path.join(CSRC, "emd_ragged.hip")).read()
    assert '#include "emd_ragged_plan.h"' in text
    assert re.search(r"const int grid = emd_ragged_plan\(c, off, num_cus\(\), a\.t\);", text)
    assert re.search(r"hipLaunchKernelGGL\(f, dim3\(grid\)", text)
    assert len(re.findall(r"emd_ragged_pair_of_block\(a\.t, blockIdx\.x\)", text)) == 1
    assert len(re.findall(r"emd_ragged_pair_of_point\(a\.t, t0\)", text)) == 3          # init, CalcDist, backward
    assert re.search(r"ws_alloc\(L, kWsEmdRagged, st\)", text)
    assert "kWsEmdRagged = 45" in open(os.path.join(CSRC, "common.h")).read()
    # no waiting across workgroups: no ticket, no spin, no scoped fetch-add
    assert not re.search(r"__hip_atomic_fetch_add|while\s*\(\s*__hip_atomic_load", text)
