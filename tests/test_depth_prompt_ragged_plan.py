"""What a genpc_depth_prompt_ragged call does (csrc/depth_prompt_ragged_plan.h), without a GPU: the header is plain C++ and is
checked by a stand-alone program under the address and undefined-behaviour sanitizers (tests/depth_prompt_ragged_plan_check.cpp;
nothing loaded into Python is sanitized) -- the limits, the item numbering, the launch count, the refusal of an empty scan.
That the entry point launches what the header counts, and that the projection arithmetic is stated once for project.hip and
the new file, is checked as text."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genpc_amd", "csrc")


def _code(text):
    return "\n".join(l.split("//")[0] for l in text.splitlines())


def test_depth_prompt_ragged_plan_program_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "depth_prompt_ragged_plan_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", CSRC, os.path.join(ROOT, "tests", "depth_prompt_ragged_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "depth_prompt_ragged_plan_check: ok" in r.stdout, r.stdout


def test_plan_header_needs_no_hip():
    text = open(os.path.join(CSRC, "depth_prompt_ragged_plan.h")).read()
    assert not re.search(r"#include\s*[<\"]hip|__device__|__global__|#include\s*\"(common|project_math)\.h\"", text)
    assert re.findall(r"#include\s*(\S+)", text) == ["<stddef.h>", '"ragged_offsets.h"']


def test_the_call_launches_what_the_header_counts():
    text = open(os.path.join(CSRC, "depth_prompt_ragged.hip")).read()
    head = open(os.path.join(CSRC, "depth_prompt_ragged_plan.h")).read()
    call = _code(text[text.index("GENPC_API int genpc_depth_prompt_ragged("):text.index("GENPC_API int genpc_depth_prompt_ragged_plan(")])
    assert re.search(r"constexpr\s+int\s+kDpLaunches\s*=\s*4\s*;", head) and re.search(r"constexpr\s+int\s+kDpMemsets\s*=\s*1\s*;", head)
    assert len(re.findall(r"hipLaunchKernelGGL\(", call)) == 4 and len(re.findall(r"hipMemsetAsync\(", call)) == 1
    assert not re.search(r"\bfor\s*\(|\bwhile\s*\(", call)                 # no loop over the scans: the count does not depend on c
    assert re.search(r"ws_alloc\(L, kWsDepthPromptRagged, st\)", call) and "kWsDepthPromptRagged = 54" in open(os.path.join(CSRC, "common.h")).read()
    assert "depth_prompt_ragged_fault(" in call and "depth_prompt_ragged_plan(" in call and "ragged_pad_copy(" in call
    gather = _code(text[text.index("GENPC_API int genpc_gather_colors_ragged("):])
    assert len(re.findall(r"hipLaunchKernelGGL\(", gather)) == 1
    code = _code(text)
    assert not re.search(r"atomicAdd\s*\(", code) and "asm" not in code                      # integer minima / maxima only
    assert "four launches" in open(os.path.join(ROOT, "include", "genpc_hip.h")).read().lower()


def test_the_projection_arithmetic_is_stated_once():
    shared = _code(open(os.path.join(CSRC, "project_math.h")).read())
    old = _code(open(os.path.join(CSRC, "project.hip")).read())
    new = _code(open(os.path.join(CSRC, "depth_prompt_ragged.hip")).read())
    for name in ("f2key", "key2f", "project_point", "project_box_centre", "project_rescale", "uv_pixel"):
        assert len(re.findall(r"__device__ __forceinline__ \w+ %s\(" % name, shared)) == 1, name
        assert not re.search(r"__forceinline__ \w+ %s\(" % name, old + new), name
        assert re.search(r"\b%s\(" % name, old) and re.search(r"\b%s\(" % name, new), name
    assert '#include "project_math.h"' in old and '#include "project_math.h"' in new
    # the rescale statement and the pixel clip appear in neither file any more
    assert "padmul), 0.5f)" not in old + new and "clip_max ? clip_max" not in old + new
