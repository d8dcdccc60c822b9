"""How a ragged ICP call is split (csrc/icp_ragged_plan.h), without a GPU: the header is plain C++ and is checked by a
stand-alone program under the address and undefined-behaviour sanitizers (tests/icp_ragged_plan_check.cpp; nothing loaded into
Python is sanitized); that the entry point and the kernels use it, and state the solve once, is checked as text."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genpc_amd", "csrc")


def test_icp_ragged_plan_program_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "icp_ragged_plan_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", CSRC, os.path.join(ROOT, "tests", "icp_ragged_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "icp_ragged_plan_check: ok" in r.stdout, r.stdout


def test_icp_ragged_plan_header_needs_no_hip():
    text = open(os.path.join(CSRC, "icp_ragged_plan.h")).read()
    assert not re.search(r"#include\s*[<\"]hip|__device__|__global__|#include\s*\"(common|nn|grid)\.h\"", text)
    assert re.findall(r"#include\s*(\S+)", text) == ['"icp_plan.h"']


def _body(text, head):
    """The text of the function that starts with `head`, braces matched."""
    i = text.index(head)
    j = text.index("{", i)
    depth, k = 0, j
    while True:
        depth += {"{": 1, "}": -1}.get(text[k], 0)
        k += 1
        if depth == 0:
            return text[i:k]


def test_the_call_reads_the_plan_and_the_solve_is_stated_once():
    icp = open(os.path.join(CSRC, "icp.hip")).read()
    call = _body(icp, "GENPC_API int genpc_icp_batch_ragged(")
    code = "\n".join(l.split("//")[0] for l in call.splitlines())
    assert "icp_ragged_plan(c, toff)" in code and re.search(r"lds\s*=\s*\(size_t\)\s*plan\.lds_bytes", code)
    for word in ("icp_fused_lds", "kFFixed", "kFLds", "kFCells", "kFIndexLimit", "8192", "4096", "2048", "160"):
        assert word not in code, word
    assert len(re.findall(r"dim3\(k\), dim3\(kFT\), lds, st, a\)", code)) == 2              # one launch, in either arithmetic mode
    assert len(re.findall(r"\bgenpc_icp_batch\(", code)) == 1                                # the loop pairs: the existing call
    assert "genpc::icp_ragged_plan" in _body(icp, "GENPC_API int genpc_icp_ragged_plan(") or "icp_ragged_plan(c, toff)" in _body(icp, "GENPC_API int genpc_icp_ragged_plan(")
    # both kernels are the one device function and nothing else
    for name in ("icp_fused_kernel", "icp_fused_ragged_kernel"):
        body = _body(icp, "void %s(" % name)
        assert len(re.findall(r"icp_fused_solve<FMA>\(", body)) == 1, name
        assert "__shared__" not in body and "for (int pass" not in body, name
    assert len(re.findall(r"for \(int pass = 0; pass <= max_iter; pass\+\+\)", _body(icp, "void icp_fused_solve("))) == 1
    ragged = _body(icp, "void icp_fused_ragged_kernel(")
    assert "icp_plan(nt)" in ragged and "plan.cells" in ragged
