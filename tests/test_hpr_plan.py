"""The plan of a hidden-point-removal call (csrc/hpr_plan.h): one kernel or two, what the first kernel takes, the sort's key bits,
the polygon stores, every grid and the element count of every piece of the workspace.  No GPU: the header is plain C++ and is
checked by a stand-alone program -- a table of asks with the plans they must give, and properties over a sweep of shapes, CU counts
and switches -- under the address and undefined-behaviour sanitizers; that hpr_run decides nothing besides, that the plan's
constants are defined once and that the status words and work lines are named is checked as text, and the exported
genpc_hpr_plan -- what tests/test_gpu_hpr_forms.py asks about its shapes -- is the same function."""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import pytest

from test_pose_plan import _body

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genpc_amd", "csrc")
SWITCHES = ("GENPC_HPR_SPLIT", "GENPC_HPR_NOCULL", "GENPC_HPR_PARK_MB", "GENPC_HPR_HOME_TILES", "GENPC_HPR_HOME_CHUNKS", "GENPC_HPR_DECIDE_KERNEL")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("hpr_plan") / "hpr_plan_check")
    # (the sanitizers' runtimes linked statically, as in tests/test_nn_plan.py)
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", CSRC, os.path.join(ROOT, "tests", "hpr_plan_check.cpp"), "-o", exe], check=True)
    return exe


def test_hpr_plan_program_under_sanitizers(program):
    r = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "hpr_plan_check: ok" in r.stdout, r.stdout


def test_hpr_plan_header_needs_no_hip():
    text = open(os.path.join(CSRC, "hpr_plan.h")).read()
    assert not re.search(r"#include\s*[<\"]hip|__device__|__global__|#include\s*\"(common|hpr)\.h\"|getenv|tune_env|num_cus", text)
    assert re.findall(r"#include\s*(\S+)", text) == ["<algorithm>"]


def _code(text):
    return "\n".join(l.split("//")[0] for l in text.splitlines())


def _hpr_files():
    return sorted(glob.glob(os.path.join(CSRC, "hpr*.hip")))


def test_hpr_run_reads_the_plan():
    """hpr_run validates, asks hpr_plan once, carves the layout from the plan's sizes and calls the launchers: it compares no size
    with a threshold and rounds nothing; the switches and the CU count are read where the ask is filled and nowhere else."""
    hpr = open(os.path.join(CSRC, "hpr.hip")).read()
    run = _code(_body(hpr, "static int hpr_run("))
    assert len(re.findall(r"\bhpr_plan\(", run)) == 1
    for word in ("num_cus", "tune_env", "ceil_div", "kHprRimTiles", "100000", "<< 20", "& ~7", "std::min", "std::max"):
        assert word not in run, word
    assert len(_body(hpr, "static int hpr_run(").splitlines()) < 90
    ask = _body(hpr, "static HprAsk hpr_ask(")
    assert len(re.findall(r"\bnum_cus\(\)", _code(hpr))) == 1 and "num_cus()" in ask
    assert len(re.findall(r"\btune_env\(", _code(hpr))) == len(re.findall(r"\btune_env\(", _code(ask))) == len(SWITCHES)
    for name in SWITCHES:
        assert '"%s"' % name in ask, name
    for path in _hpr_files() + [os.path.join(CSRC, "hpr.h")]:
        if not path.endswith("/hpr.hip"):
            code = _code(open(path).read())
            assert "num_cus" not in code and "tune_env" not in code and "hpr_plan(" not in code, path
    # the launches are in the passes' files, in the order hpr_run calls them
    order = [run.index(w) for w in ("hpr_launch_order(", "hpr_launch_accept(", "hpr_launch_first(", "hpr_launch_wave(")]
    assert order == sorted(order) and "hipLaunchKernelGGL" not in run
    exported = _body(hpr, "GENPC_API int genpc_hpr_plan(")
    assert "hpr_plan(ask)" in exported and "hpr_ask(c, n, best_only, cus)" in exported


def test_the_plan_s_constants_are_defined_once():
    plan_h = open(os.path.join(CSRC, "hpr_plan.h")).read()
    others = _hpr_files() + [os.path.join(CSRC, "hpr.h")]
    for name in ("kHprThreads", "kHprMaxV", "kHprOverCap", "kHprRimTiles", "kHprWorkLine", "kHprWorkWords", "kHprDecideWaves", "kHprWalkWaves", "kHprLargeWaves"):
        assert len(re.findall(r"\b%s\s*=" % name, _code(plan_h))) == 1, name
        for path in others:
            assert not re.search(r"\b%s\s*=[^=]" % name, _code(open(path).read())), (name, path)
    # the per-CU wave counts are numbers in the plan alone
    for path in others:
        assert not re.search(r"grid_of\(|\*\s*cus\b", _code(open(path).read())), path
    assert re.search(r"kHprDecideWaves = 64, kHprWalkWaves = 40, kHprLargeWaves = 5\b", plan_h)
    assert '#include "hpr_plan.h"' in open(os.path.join(CSRC, "hpr.h")).read()


def test_status_words_and_work_lines_are_named():
    """Outside hpr.h no file indexes the status header or the work counters with an integer literal; hpr.h names the words."""
    for path in _hpr_files():
        code = _code(open(path).read())
        for m in re.finditer(r"\b(?:status|work|st)\s*(?:\[|\+)\s*\(?\s*\d[^;\n]*", code):
            raise AssertionError((os.path.basename(path), m.group(0)))
        assert not re.search(r"no_cull\s*&\s*\(?\s*\d", code), path
    hdr = open(os.path.join(CSRC, "hpr.h")).read()
    for word, value in (("kHprStListed", 0), ("kHprStError", 1), ("kHprStParked", 2), ("kHprStOver128", 3), ("kHprStOverCap", 4), ("kHprStUndecided", 5),
                        ("kHprStBounds", 16), ("kHprStSegFill", 32), ("kHprStSegs", 48), ("kHprWorkFirstTry", 0), ("kHprWorkContinue", 8),
                        ("kHprWorkListed", 9), ("kHprWorkLarge", 10), ("kHprWorkGlobal", 11)):
        assert re.search(r"\b%s = %d," % (word, value), hdr), word
    assert hdr.lstrip().startswith("//") and re.search(r"^#pragma clang fp contract\(off\)", hdr, re.M)
    assert hdr.index("#pragma clang fp contract(off)") < hdr.index("#include")


def test_exported_plan_is_the_header_s(program):
    """genpc_hpr_plan through ctypes, with a CU count given (no GPU is touched), against the table's literals: every row that
    sets no switch."""
    from genpc_amd import _lib
    for env in SWITCHES:
        assert not os.environ.get(env), "%s is set: the table's rows are for the defaults" % env
    r = subprocess.run([program, "--exported"], stdout=subprocess.PIPE, text=True, timeout=60, check=True)
    rows = [l for l in r.stdout.splitlines() if " : " in l]
    assert len(rows) >= 12 and any(l.split()[3] == "64" for l in rows)
    failures = []
    for l in rows:
        ask, want = (list(map(int, part.split())) for part in l.split(" : "))
        out = (ctypes.c_int * 24)(*([-1] * 24))
        if _lib.lib.genpc_hpr_plan(*ask, ctypes.cast(out, ctypes.c_void_p)) != 1 or list(out) != want:
            failures.append((l, list(out)))
    assert not failures, failures[:3]
    out = (ctypes.c_int * 24)()
    assert _lib.lib.genpc_hpr_plan(1, 100, 0, 256, None) == -1
    assert _lib.lib.genpc_hpr_plan(-1, 100, 0, 256, ctypes.cast(out, ctypes.c_void_p)) == -1
