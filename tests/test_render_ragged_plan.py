"""The shape of a ragged render call (csrc/render_ragged_plan.h): every refusal, the bound on s, the largest element, both
launches' grids and the scratch's element counts, as a pure function.  No GPU: the header is plain C++ and is checked by a
stand-alone program under the address and undefined-behaviour sanitizers; that the entry points decide nothing besides is checked
as text, and the exported genpc_render_ragged_plan is the same function."""
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
    exe = str(tmp_path_factory.mktemp("render_ragged_plan") / "render_ragged_plan_check")
    # (the sanitizers' runtimes linked statically, as in tests/test_fps_plan.py)
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", CSRC, os.path.join(ROOT, "tests", "render_ragged_plan_check.cpp"), "-o", exe], check=True)
    return exe


def test_render_ragged_plan_program_under_sanitizers(program):
    r = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "render_ragged_plan_check: ok" in r.stdout, r.stdout


def test_render_ragged_plan_header_needs_no_hip():
    text = open(os.path.join(CSRC, "render_ragged_plan.h")).read()
    assert not re.search(r"#include\s*[<\"]hip|__device__|__global__|#include\s*\"(common|mask|pose)\.h\"", text)
    assert re.findall(r"#include\s*(\S+)", text) == ["<stddef.h>", "<stdio.h>", "<algorithm>", '"pose_plan.h"', '"ragged_offsets.h"']
    for name in ("pose_plan.h", "ragged_offsets.h"):          # ... and neither do the two it includes
        assert not re.search(r"#include\s*[<\"]hip", open(os.path.join(CSRC, name)).read()), name


def _code(text):
    return "\n".join(l.split("//")[0] for l in text.splitlines())


def test_the_entry_points_read_the_plan():
    """Both entry points and the exported plan fill a RenderRaggedAsk, call render_ragged_plan once and refuse with its words; no
    comparison of an argument and no grid arithmetic stands in their bodies."""
    src = open(os.path.join(CSRC, "render_grad.hip")).read()
    for fn in ("genpc_render_points_ragged", "genpc_render_points_ragged_backward", "genpc_render_ragged_plan"):
        body = _code(_body(src, "GENPC_API int %s(" % fn))
        assert len(re.findall(r"\brender_ragged_plan\(ask\)", body)) == 1, fn
        assert "render_ragged_refuse(fn, plan)" in body, fn
        for word in ("384", "8192", "1ll << 28", "1 << 28", "lin_grid", "ragged_offsets_fault", "kRenderSub", "kRenderRaggedMax + "):
            assert word not in body, (fn, word)
        assert not re.search(r"\b(s|size|blend)\s*(<=?|>=?|==|!=)\s*\d", body), fn
        assert not re.search(r"\bradius\[", body), fn
    fwd = _code(_body(src, "GENPC_API int genpc_render_points_ragged("))
    for field in ("plan.g_proj", "plan.g_pix", "plan.nmax", "plan.nmax_piece", "plan.table_ints", "plan.table_floats"):
        assert field in fwd, field
    assert "launch_mask_splat(plan.s, plan.nmax," in fwd and "RenderBlendScope scope(blend)" in fwd and "false" in fwd
    bwd = _code(_body(src, "GENPC_API int genpc_render_points_ragged_backward("))
    for field in ("plan.nothing", "plan.gx", "plan.grad_blocks", "plan.w_pixels", "plan.g_pix"):
        assert field in bwd, field
    # the tables go to the device by value in a kernel's arguments: no host-to-device copy in either entry point
    for body in (fwd, bwd, _code(_body(src, "static int render_ragged_tables("))):
        assert "hipMemcpyHostToDevice" not in body and "hipMemcpy(" not in body
    assert "ragged_pad_copy(a.off, off, s)" in _body(src, "static int render_ragged_tables(")
    # the backward has no atomics, and the gather's loop is stated once
    assert "atomic" not in _code(_body(src, "__device__ __forceinline__ void render_grad_points_body("))
    assert len(re.findall(r"render_grad_points_body<BLEND, COL>\(", _code(src))) == 2
    assert len(re.findall(r"__builtin_amdgcn_rcpf", _code(src))) == 1


def test_exported_plan_is_the_header_s(program):
    """genpc_render_ragged_plan through ctypes (no GPU is touched) equals the header's values, refusals included."""
    from genpc_amd import _lib

    def exported(size, blend, radius, ns):
        off = [0]
        for n in ns:
            off.append(off[-1] + n)
        o = (ctypes.c_int * len(off))(*off)
        r = (ctypes.c_float * max(1, len(ns)))(*([radius] * len(ns)))
        out = (ctypes.c_int * 12)(*([-7] * 12))
        rc = _lib.lib.genpc_render_ragged_plan(len(ns), ctypes.cast(o, ctypes.c_void_p), ctypes.cast(r, ctypes.c_void_p), size, blend,
                                               ctypes.cast(out, ctypes.c_void_p))
        return rc, list(out)

    def header(size, blend, radius, ns):
        r = subprocess.run([program, str(size), str(blend), repr(radius)] + [str(n) for n in ns], stdout=subprocess.PIPE, text=True, check=True,
                           timeout=60)
        return r.stdout.split()

    for size, blend, radius, ns in ((64, 1, 0.02, [5]), (96, 0, 0.01, [0, 0, 0]), (224, 1, 0.005, [2451, 31, 0, 257]),
                                    (64, 0, 0.02, [1, 32, 33, 256, 257]), (8192, 1, 0.02, [300000, 7]), (64, 1, 0.02, [3] * 384)):
        rc, got = exported(size, blend, radius, ns)
        want = header(size, blend, radius, ns)
        assert rc == 1 and got == [int(v) for v in want], (size, blend, ns, got, want)
    for size, blend, radius, ns, words in ((64, 1, 0.02, [3] * 385, "more than 384 elements in one call"), (0, 1, 0.02, [5], "size must be in 1 .. 8192"),
                                           (64, 2, 0.02, [5], "blend must be 0 or 1"),
                                           (64, 1, 0.0, [5, 6], "the radius of every element must be positive (element 0)"),
                                           (8192, 1, 0.02, [1] * 5, "off[s] and s * size * size must not exceed 2^28")):
        rc, got = exported(size, blend, radius, ns)
        want = header(size, blend, radius, ns)
        assert rc == -1 and want[0] == "refused" and " ".join(want[2:]) == words, (ns, want)
        assert _lib.last_error() == "genpc_render_ragged_plan: " + words
        assert got[0] == 384 and got[1] == int(want[1]) and got[2:] == [0] * 10
    assert _lib.lib.genpc_render_ragged_plan(1, None, None, 64, 1, None) == -1
    out = (ctypes.c_int * 12)()
    assert _lib.lib.genpc_render_ragged_plan(1, None, None, 64, 1, ctypes.cast(out, ctypes.c_void_p)) == -1
    assert _lib.last_error() == "genpc_render_ragged_plan: off is null"
    assert _lib.lib.genpc_render_ragged_plan(0, None, None, 64, 1, ctypes.cast(out, ctypes.c_void_p)) == -1
    assert _lib.last_error() == "genpc_render_ragged_plan: s must be positive"


def test_the_entry_points_refuse_by_name_before_anything_else():
    """Both entry points return -1 with the plan's words before any device call (no GPU is touched: a refused call enqueues
    nothing).  The data pointers are host buffers -- valid, and never read."""
    from genpc_amd import _lib
    L = _lib.lib
    data = (ctypes.c_float * 512)(*([7.25] * 512))
    d = ctypes.cast(data, ctypes.c_void_p)
    vp = lambda a: None if a is None else ctypes.cast(a, ctypes.c_void_p)
    ints = lambda v: (ctypes.c_int * len(v))(*v)
    floats = lambda v: (ctypes.c_float * len(v))(*v)

    def fwd(s=2, off=(0, 3, 8), radius=(0.02, 0.03), size=4, blend=1, pts=d, img=d):
        o, r = None if off is None else ints(off), None if radius is None else floats(radius)
        return L.genpc_render_points_ragged(s, vp(o), pts, d, vp(r), size, blend, img, d, None)

    def bwd(s=2, off=(0, 3, 8), radius=(0.02, 0.03), size=4, blend=1, pts=d, planes=d, grad_img=d, grad_pts=d):
        o, r = None if off is None else ints(off), None if radius is None else floats(radius)
        return L.genpc_render_points_ragged_backward(s, vp(o), pts, d, vp(r), size, blend, planes, grad_img, grad_pts, d, None)
    both = [(dict(s=0), "s must be positive"), (dict(s=385, off=tuple(range(386)), radius=(0.02,) * 385), "more than 384 elements in one call"),
            (dict(off=None), "off is null"), (dict(radius=None), "radius is null"), (dict(off=(2, 3, 8)), "offsets must start at 0"),
            (dict(off=(0, 5, 3)), "offsets must ascend"), (dict(radius=(0.02, -0.5)), "the radius of every element must be positive (element 1)"),
            (dict(size=0), "size must be in 1 .. 8192"), (dict(size=8193), "size must be in 1 .. 8192"), (dict(blend=3), "blend must be 0 or 1"),
            (dict(off=(0, 3, (1 << 28) + 1)), "off[s] and s * size * size must not exceed 2^28"),
            (dict(s=5, off=(0, 1, 2, 3, 4, 5), radius=(0.02,) * 5, size=8192), "off[s] and s * size * size must not exceed 2^28"),
            (dict(pts=None), "pts is null")]
    for kw, words in both + [(dict(img=None), "img is null")]:
        assert fwd(**kw) == -1 and _lib.last_error() == "genpc_render_points_ragged: " + words, kw
    for kw, words in both + [(dict(planes=None), "planes is null"), (dict(grad_img=None), "grad_img is null"), (dict(grad_pts=None), "grad_pts is null")]:
        assert bwd(**kw) == -1 and _lib.last_error() == "genpc_render_points_ragged_backward: " + words, kw
    assert bwd(off=(0, 0, 0), pts=None, planes=None, grad_img=None, grad_pts=None) == 1
    assert list(data) == [7.25] * 512
