"""Which sampler a cloud of a farthest-point-sampling call takes (csrc/fps_plan.h): the one-workgroup LDS sampler up to 24576
points, the multi-workgroup kernel up to 262144, the large sampler (csrc/fps_large.hip) up to 4194304 -- and every size the
large sampler needs.  No GPU: the header is plain C++ and is checked by a stand-alone program under the address and
undefined-behaviour sanitizers; that the entry points and fps_grid_takes decide nothing besides is checked as text, and the
exported genpc_fps_plan is the same function."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from test_pose_plan import _body

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genpc_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("fps_plan") / "fps_plan_check")
    # (the sanitizers' runtimes linked statically, as in tests/test_icp_plan.py)
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", CSRC, os.path.join(ROOT, "tests", "fps_plan_check.cpp"), "-o", exe], check=True)
    return exe


def test_fps_plan_program_under_sanitizers(program):
    r = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "fps_plan_check: ok" in r.stdout, r.stdout


def test_fps_plan_header_needs_no_hip():
    text = open(os.path.join(CSRC, "fps_plan.h")).read()
    assert not re.search(r"#include\s*[<\"]hip|__device__|__global__|#include\s*\"(common|nn|grid)\.h\"", text)
    assert re.findall(r"#include\s*(\S+)", text) == ["<stddef.h>"]


def _code(text):
    return "\n".join(l.split("//")[0] for l in text.splitlines())


def test_the_entry_points_and_the_kernels_read_the_plan():
    """genpc_fps_multi and genpc_fps_large are one body that asks fps_plan for every cloud and holds no size of its own;
    fps_grid_takes is the plan's answer; the large sampler's launcher takes its sizes from the plan."""
    fps = open(os.path.join(CSRC, "fps_call.hip")).read()
    assert "fps_call(c, n, k, xyz, out_idx, stream, 0)" in _body(fps, "GENPC_API int genpc_fps_multi(")
    assert "fps_call(c, n, k, xyz, out_idx, stream, 1)" in _body(fps, "GENPC_API int genpc_fps_large(")
    call = _code(_body(fps, "static int fps_call("))
    # the admission and the choice of sampler in fps_call, the sizes in the workspace function it calls: all ask fps_plan
    header = _code(open(os.path.join(CSRC, "fps_plan.h")).read())
    assert len(re.findall(r"fps_plan\(n\[j\], force_large\)", call)) >= 2
    assert "fps_workspace(c, n, k, sampler.data()" in call and "fps_plan(n[j], 1)" in _body(header, "inline FpsWorkspace fps_workspace(")
    for word in ("262144", "24576", "kGMaxN", "15360"):
        assert word not in call, word
    assert not re.search(r"n\[j\]\s*[<>]=?\s*\d", call)                  # no comparison of a point count with a number
    assert not re.search(r"\[[&=]?\]\s*\(", call)                         # no lambda: every decision is a function of fps_plan.h
    for name in ("fps_multi_shape(", "fps_multi_launches(", "fps_workspace(", "fps_k_pad(", "fps_seg_points("):
        assert name in call, name
    assert "genpc::fps_plan(n, force_large)" in _body(fps, "GENPC_API int genpc_fps_plan(")
    grid = _code(open(os.path.join(CSRC, "fps_grid.hip")).read())
    assert re.search(r"bool fps_grid_takes\(int n\)\s*\{\s*return fps_plan\(n, 0\)\.sampler == kFpsGrid;\s*\}", grid)
    assert "24576" not in grid
    large = _code(open(os.path.join(CSRC, "fps_large.hip")).read())
    run = _body(large, "int fps_large_run(")
    assert len(re.findall(r"fps_plan\(n\[", run)) == 2
    for field in ("p.npad", "p.chunks", "p.starts", "p.cells_target", "p.cells_max", "p.lds_bytes"):
        assert field in run, field
    assert not re.search(r"\b(4194304|262144|15360|12288)\b", large)
    # each packed field is asserted against the limits where it is defined
    plan = open(os.path.join(CSRC, "fps_plan.h")).read()
    for name in ("kFpsLargeCellBits", "kFpsLargePosBits", "kFpsLargeIndexBits", "kFpsLargeSampleBits"):
        assert re.search(r"static_assert\([^;]*%s" % name, plan), name
        assert name in large or name == "kFpsLargeSampleBits", name


def test_the_register_classes_are_stated_once():
    """The boundaries 2 / 4 / 8 / 12 / 16 / 24 of fps_kernel's instantiations stand in fps_plan.h alone; fps.hip builds ONE table of
    instantiations from them, and both the launch and the occupancy query go through it -- no file launches fps_kernel by name."""
    literal = re.compile(r"2\s*,\s*4\s*,\s*8\s*,\s*12\s*,\s*16\s*,\s*24")
    holders = [f for f in sorted(os.listdir(CSRC)) if literal.search(_code(open(os.path.join(CSRC, f)).read()))]
    assert holders == ["fps_plan.h"], holders
    plan = _code(open(os.path.join(CSRC, "fps_plan.h")).read())
    assert len(literal.findall(plan)) == 1 and re.search(r"kFpsClassPoints\[kFpsClasses\]\s*=\s*\{2, 4, 8, 12, 16, 24\}", plan)
    assert "kFpsClassPoints[cls]" in _body(plan, "inline int fps_class(")
    fps = _code(open(os.path.join(CSRC, "fps.hip")).read())
    table = _body(fps, "static FpsKernel fps_kernel_of(")
    assert [int(i) for i in re.findall(r"fps_kernel<FMA, kFpsClassPoints\[(\d)\]>", table)] == [0, 1, 2, 3, 4, 5]
    # an instantiation is named in the table and nowhere else; switch statements over R or the class are gone
    for name in ("fps.hip", "fps_call.hip", "fps_verify.hip"):
        text = _code(open(os.path.join(CSRC, name)).read())
        outside = text.replace(table, "") if name == "fps.hip" else text
        assert "hipLaunchKernelGGL((fps_kernel<" not in outside, name
        assert not re.search(r"fps_kernel<\s*(FMA|[01])\s*,", outside), name
        assert not re.search(r"case 1[0-9]:|R <= \d", outside), name
    assert re.search(r"hipOccupancyMaxActiveBlocksPerMultiprocessor\([^;]*fps_kernel_of<1>\(cls\)[^;]*fps_kernel_of<0>\(cls\)", _body(fps, "bool fps_device("))
    run = _body(fps, "int fps_multi_run(")
    assert re.search(r"fps_kernel_of<1>\(fps_class\(la\.rmax\)\)\s*:\s*fps_kernel_of<0>\(fps_class\(la\.rmax\)\)", run)
    assert "hipLaunchKernelGGL(kernel, dim3(la.wmax, la.count), dim3(kFBlock)" in run
    # one fill of a job-table entry, in the shared header
    shared = _code(open(os.path.join(CSRC, "fps.h")).read())
    fills = sum(len(re.findall(r"jobs\.pdist\[\w+\]\s*=", _code(open(os.path.join(CSRC, f)).read())))
                for f in ("fps.h", "fps.hip", "fps_call.hip", "fps_verify.hip"))
    assert fills == 1 and "jobs.pdist[q] = c.pdist[j];" in _body(shared, "inline void fps_fill_job(")
    # nothing is declared by hand any more
    for name in ("fps.hip", "fps_call.hip", "fps_verify.hip", "fps_grid.hip", "fps_large.hip", "pose.hip"):
        text = _code(open(os.path.join(CSRC, name)).read())
        assert '#include "fps.h"' in text, name
        assert not re.search(r"^\s*(bool|void|int)\s+(persist_reserve|persist_commit|emd_auction_capacity|fps_deferred_prepare)\([^)]*\);", text, re.M), name


def test_exported_plan_is_the_header_s(program):
    """genpc_fps_plan through ctypes (no GPU is touched) equals the header's values at the boundaries."""
    from genpc_amd import _lib

    def plan(n, force):
        out = (ctypes.c_int * 8)(*([-7] * 8))
        rc = _lib.lib.genpc_fps_plan(n, force, ctypes.cast(out, ctypes.c_void_p))
        return rc, tuple(out)

    def header(n, force):
        r = subprocess.run([program, str(n), str(force)], stdout=subprocess.PIPE, text=True, check=True, timeout=60)
        return tuple(int(v) for v in r.stdout.split())

    for n in (1, 24576, 24577, 262144, 262145, 1000000, 4194304, 4194305, 0):
        for force in (0, 1):
            rc, got = plan(n, force)
            assert got == header(n, force), (n, force)
            assert rc == (1 if 1 <= n <= 4194304 else -1)
    assert [plan(n, 0)[1][0] for n in (24576, 24577, 262144, 262145, 4194304, 4194305)] == [0, 1, 1, 2, 2, -1]
    assert plan(1, 1)[1][0] == 2
    assert plan(262145, 0)[1][1:] == (15360, 12288, 262272, 32784, 15361, 4096 * 8 + 1792 * 4 + 384 * 4, 0)
    assert _lib.lib.genpc_fps_plan(100, 0, None) == -1
