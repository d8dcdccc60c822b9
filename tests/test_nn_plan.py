"""The plan of a nearest-neighbour call (csrc/nn_plan.h): kernel family, Q / R, bookkeeping unit, lists per lane, slice length,
the f16 filter's block form, every grid and workspace size.  No GPU: the header is plain C++ and is checked by a stand-alone
program -- a table of asks with the plans they must give, and properties over a sweep of shapes and CU counts -- under the address
and undefined-behaviour sanitizers; that nn_forward and the two launchers decide nothing besides is checked as text, and the
exported genpc_nn_plan -- what tests/test_gpu_nn_forms.py takes its shapes from -- is the same function."""
import ctypes
import os
import re
import shutil
import subprocess
import threading

import pytest

from test_pose_plan import _body

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genpc_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("nn_plan") / "nn_plan_check")
    # (the sanitizers' runtimes linked statically, as in tests/test_pose_plan.py)
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", CSRC, os.path.join(ROOT, "tests", "nn_plan_check.cpp"), "-o", exe], check=True)
    return exe


def test_nn_plan_program_under_sanitizers(program):
    r = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "nn_plan_check: ok" in r.stdout, r.stdout


def test_nn_plan_header_needs_no_hip():
    text = open(os.path.join(CSRC, "nn_plan.h")).read()
    assert not re.search(r"#include\s*[<\"]hip|__device__|__global__|#include\s*\"(common|nn|grid)\.h\"|getenv|tune_env|num_cus", text)
    assert re.findall(r"#include\s*(\S+)", text) == ["<algorithm>"]


def _code(text):
    return "\n".join(l.split("//")[0] for l in text.splitlines())


def test_the_call_and_the_launchers_read_the_plan():
    """nn_forward asks nn_plan and only allocates, runs the duplicate policy, fills NNArgs and launches; launch_nn_f16 and
    launch_nn_finish map the plan to a template instance.  None of them asks for the CU count, rounds a size up or compares
    one with a threshold, and the retired codes (`tight`, `big`, the renumbered `path`) are gone."""
    chamfer = open(os.path.join(CSRC, "chamfer.hip")).read()
    f16 = open(os.path.join(CSRC, "nn_f16.hip")).read()
    finish = open(os.path.join(CSRC, "nn_finish.hip")).read()
    fwd = _code(_body(chamfer, "int nn_forward(int b, int ndir"))
    assert "nn_plan(ask)" in fwd
    bodies = {"nn_forward": fwd, "launch_nn_f16": _code(_body(f16, "int launch_nn_f16(")), "launch_main": _code(_body(f16, "static void launch_main(")),
              "launch_nn_finish": _code(_body(finish, "int launch_nn_finish("))}
    for name, code in bodies.items():
        for word in ("num_cus", "ceil_div", "nn_ceil", "kChunk", "kFQ", "want_blocks", "pairs", "cfg.", "t_tune_path", "slice_len >", "tight", "big", "path",
                     "unsplit", "6e6", "2e8", "8192", "1 << 25"):
            assert word not in code, (name, word)
        assert not re.search(r"\b(1024|2048|512|192|128|64)\b", code.replace("1 << 16", "")) or name == "nn_forward", name
    # (nn_forward's own numbers are its workspace's: the zeroed prefix and the duplicate policy's)
    assert set(re.findall(r"\b(?:1024|2048|512|192|128)\b", fwd)) <= {"512", "2048"}          # hooks 512 and 2048 of genpc_nn_tune
    # the CU count enters the nearest-neighbour host code once, where the ask is filled
    assert len(re.findall(r"\bnum_cus\(\)", _code(chamfer))) == 1 and "num_cus()" in _body(chamfer, "static NNAsk nn_ask(")
    assert "num_cus" not in _code(f16) and "num_cus" not in _code(finish)
    # what is launched is what the plan says
    assert len(re.findall(r"\bplan\.form == kNN(?:Wide|Tile2048|ThreeWave)\b", bodies["launch_main"])) == 3
    assert re.search(r"dim3\(\(unsigned\)plan\.fin_blocks\)", bodies["launch_nn_finish"]) and "plan.early" in bodies["launch_nn_finish"]
    # the constants of the plan are defined in nn_plan.h alone
    plan_h = open(os.path.join(CSRC, "nn_plan.h")).read()
    for name in ("kChunk", "kBlock", "kMaxLists", "kHTile", "kFQ"):
        assert re.search(r"constexpr\s+int\s+%s\b" % name, plan_h), name
        for other in ("chamfer.hip", "nn_f16.hip", "nn_finish.hip", "nn.h"):
            assert not re.search(r"constexpr\s+int\s+%s\b" % name, open(os.path.join(CSRC, other)).read()), (name, other)
    exported = _body(chamfer, "GENPC_API int genpc_nn_plan(")
    assert "nn_plan(ask)" in exported and "nn_ask(b, cus)" in exported


def test_exported_plan_is_the_header_s(program):
    """genpc_nn_plan through ctypes, with a CU count given (no GPU is touched), against the table's literals: every row that has
    the shape of a genpc_chamfer_forward / genpc_nm_distance call, the forced family set with genpc_nn_tune."""
    from genpc_amd import _lib
    r = subprocess.run([program, "--exported"], stdout=subprocess.PIPE, text=True, timeout=60, check=True)
    rows = [l for l in r.stdout.splitlines() if " : " in l]
    assert len(rows) >= 20 and any(l.split()[4] == "64" for l in rows) and sum(l.split()[4] == "256" for l in rows) >= 15
    for env in ("GENPC_NN_PATH", "GENPC_NN_R", "GENPC_NN_Q", "GENPC_NN_U", "GENPC_NN_WPS"):
        assert not os.environ.get(env), "%s is set: the table's rows are for the defaults" % env
    lib = _lib.lib
    failures = []

    def compare():
        # (in a thread of its own: genpc_nn_tune's family is the calling thread's and cannot be unset, and the rows without a
        # forced family need a thread that never forced one)
        try:
            for l in rows:
                ask, want = (list(map(int, part.split())) for part in l.split(" : "))
                b, n, m, ndir, cus, forced = ask
                out = (ctypes.c_int * 16)(*([-1] * 16))
                lib.genpc_nn_tune(forced, -1)
                if lib.genpc_nn_plan(b, n, m, ndir, cus, ctypes.cast(out, ctypes.c_void_p)) != 1 or list(out) != want:
                    failures.append((l, list(out)))
        except Exception as e:          # noqa: BLE001 -- reported below, in the test's own thread
            failures.append(repr(e))

    # rows without a forced family first: once forced, a thread stays forced
    rows.sort(key=lambda l: int(l.split()[5]) >= 0)
    t = threading.Thread(target=compare)
    t.start()
    t.join()
    assert not failures, failures[:3]
    out = (ctypes.c_int * 16)()
    assert lib.genpc_nn_plan(1, 100, 100, 2, 256, None) == -1
    assert lib.genpc_nn_plan(1, 100, 100, 3, 256, ctypes.cast(out, ctypes.c_void_p)) == -1
