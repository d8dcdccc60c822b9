"""The scratch layouts of the host code (csrc/ws_layout.h, the slot table of csrc/common.h).  No GPU: the helper is plain
C++ and is checked by a stand-alone program under the address and undefined-behaviour sanitizers; the call sites are
checked as text."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genpc_amd", "csrc")


def _hip_sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))


def test_ws_layout_program_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "ws_layout_check")
    # (the sanitizers' runtimes linked statically -- clang's default, g++'s on request -- so that the program is checked the
    # same way whatever else the process environment loads beside it)
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", CSRC, os.path.join(ROOT, "tests", "ws_layout_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0 and "ws_layout_check: ok" in r.stdout, r.stdout


def test_ws_layout_header_needs_no_hip():
    text = open(os.path.join(CSRC, "ws_layout.h")).read()
    assert not re.search(r"#include\s*[<\"]hip|__device__|__global__|#include\s*\"common.h\"", text)


def test_no_literal_workspace_slot():
    """Every slot of the pool is an enumerator of common.h's Ws table: no call names one by number."""
    named = 0
    for f in _hip_sources():
        text = open(os.path.join(CSRC, f)).read()
        for m in re.finditer(r"\bworkspace\(\s*(\w+)|\bws_alloc\(\s*\w+\s*,\s*(\w+)", text):
            slot = m.group(1) or m.group(2)
            assert not slot[0].isdigit(), (f, m.group(0))
            named += slot.startswith("kWs")
    assert named >= 30, named          # (the search still finds the calls: 37 when this was written)


def test_one_round_up():
    """The 256-byte round-up is ws_layout.h's.  (mesh_sample.hip lays out its caller's buffer, whose size is public ABI;
    probe.hip's `+ 255` counts blocks.)"""
    for f in sorted(os.listdir(CSRC)):
        if f in ("ws_layout.h", "mesh_sample.hip", "probe.hip"):
            continue
        for i, line in enumerate(open(os.path.join(CSRC, f)), 1):
            assert "+ 255" not in line, "%s:%d: %s" % (f, i, line.strip())
