"""How a ragged scale-search call treats a pair (csrc/scale_search_ragged_plan.h), without a GPU: the header is plain C++ and is
checked by a stand-alone program under the address and undefined-behaviour sanitizers (tests/scale_search_ragged_plan_check.cpp;
nothing loaded into Python is sanitized); that the entry point and the kernel read it, and that the score's sums are stated
once (csrc/cd_score.h) for cd_score_kernel and the new kernel alike, is checked as text."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genpc_amd", "csrc")


def test_scale_search_ragged_plan_program_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "scale_search_ragged_plan_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", CSRC, os.path.join(ROOT, "tests", "scale_search_ragged_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "scale_search_ragged_plan_check: ok" in r.stdout, r.stdout


def test_scale_search_ragged_plan_header_needs_no_hip():
    text = open(os.path.join(CSRC, "scale_search_ragged_plan.h")).read()
    assert not re.search(r"#include\s*[<\"]hip|__device__|__global__|#include\s*\"(common|nn|grid|cd_score)\.h\"", text)
    assert re.findall(r"#include\s*(\S+)", text) == ["<stddef.h>", '"ragged_table.h"']


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


def _code(text):
    return "\n".join(l.split("//")[0] for l in text.splitlines())


REDUCTION = r"__shfl|wave_sum63|dpp_or_zero|\(double\)\s*sqrtf|\+=\s*red\["


def test_the_sums_are_stated_once():
    """cd_score_kernel and scale_search_ragged_kernel both take each thread's share from cd_score_thread_sum and reduce through
    cd_score_reduce; neither they nor anything else in the new file adds square roots or reduces over lanes by itself."""
    icp = open(os.path.join(CSRC, "icp.hip")).read()
    new = _code(open(os.path.join(CSRC, "scale_search_ragged.hip")).read())
    shared = _code(open(os.path.join(CSRC, "cd_score.h")).read())
    old_kernel = _code(_body(icp, "void cd_score_kernel("))
    new_kernel = _body(new, "void scale_search_ragged_kernel(")
    for name, body in (("cd_score_kernel", old_kernel), ("scale_search_ragged_kernel", new_kernel)):
        assert len(re.findall(r"\bcd_score_thread_sum\(", body)) == 2, name
        assert len(re.findall(r"\bcd_score_reduce\(", body)) == 1, name
        assert not re.search(REDUCTION, body), name
    assert not re.search(REDUCTION, new)
    assert re.search(r"constexpr\s+int\s+kIBlock\s*=\s*256\s*;", shared) and not re.search(r"constexpr\s+\w+\s+kIBlock\b", icp + new)
    assert len(re.findall(r"\(double\)\s*sqrtf", shared)) == 1 and len(re.findall(r"__shfl_xor", shared)) == 2
    assert '#include "cd_score.h"' in icp and '#include "cd_score.h"' in new


def test_the_call_and_the_kernel_read_the_plan():
    new = open(os.path.join(CSRC, "scale_search_ragged.hip")).read()
    call = _code(_body(new, "GENPC_API int genpc_scale_search_scores_ragged("))
    kernel = _code(_body(new, "void scale_search_ragged_kernel("))
    assert "scale_search_plan(" in call and "scale_search_plan(ns)" in kernel and "plan.cells" in kernel and "kSsFixed" in kernel
    for word in ("scale_search_lds", "kSsLds", "kSsCellsMin", "160", "1024"):
        assert word not in call and word not in kernel, word
    assert "__shared__" not in kernel.replace("extern __shared__", "")          # every byte of LDS is the plan's
    assert len(re.findall(r"dim3\(k\), dim3\(kIBlock\), lds, st, a\)", call)) == 2          # one launch, in either arithmetic mode
    assert len(re.findall(r"\blaunch_cell_grid_build_ragged\(", call)) == 1
    assert len(re.findall(r"\bgenpc_scale_search_scores\(", call)) == 1                     # the pairs that do not fit: the existing call
    assert re.search(r"ws_alloc\(L, kWsScaleSearchRagged, st\)", call)
    assert "kWsScaleSearchRagged = 47" in open(os.path.join(CSRC, "common.h")).read()
    # grid.h's own pieces, nothing restated: the box, the sizing, the scan, the cell function and the walk
    for piece in ("grid_block_box<kIBlock>(", "grid_size<16, false>(", "grid_scan_counts<kIBlock>(", "grid_cell1("):
        assert piece in kernel, piece
    assert new.count("cell_grid_shell_walk(") == 1 and "floorf" not in _code(new)
    exported = _body(new, "GENPC_API int genpc_scale_search_ragged_plan(")
    assert "scale_search_ragged_plan(c, soff)" in exported
