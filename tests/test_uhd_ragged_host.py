"""The host side of the ragged directed Hausdorff distance, without a GPU: genpc_uhd_ragged is declared, bound and exported
and the ABI version stands; what metric.uhd_ragged refuses; and csrc/ragged_items.h -- the numbering of work items of 1024
queries that csrc/uhd_ragged.hip's workgroups find their pair by -- as a stand-alone program under the address and
undefined-behaviour sanitizers (tests/uhd_ragged_table_check.cpp; nothing loaded into Python is sanitized)."""
import os
import re
import shutil
import subprocess

import pytest
import torch

from test_abi import header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genpc_amd", "csrc")


@pytest.fixture(scope="module")
def metric():
    from genpc_amd import build
    build.build(verbose=False)
    from genpc_amd import metric
    return metric


def clouds(*sizes):
    return [torch.arange(n * 3, dtype=torch.float32).reshape(n, 3) for n in sizes]


def test_genpc_uhd_ragged_is_declared_bound_and_exported(metric):
    from genpc_amd import _lib
    assert header_prototypes().get("genpc_uhd_ragged") == 8
    res, args = _lib.SIGNATURES["genpc_uhd_ragged"]
    assert len(args) == 8
    assert getattr(_lib.lib, "genpc_uhd_ragged") is not None


def test_abi_version_is_the_library_s(metric):
    from genpc_amd import _lib
    assert _lib.ABI_VERSION >= 25 and _lib.lib.genpc_abi_version() == _lib.ABI_VERSION


def test_cpu_tensors_raise(metric):
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        metric.uhd_ragged(clouds(3, 5), clouds(4, 2))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        metric.uhd_ragged((torch.zeros(8, 3), [0, 3, 8]), (torch.zeros(6, 3), [0, 4, 6]), return_witness=True)
    with pytest.raises(RuntimeError, match="GPU tensors only"):                   # float32-representable float64: only the device is wrong
        metric.uhd_ragged([c.double() for c in clouds(3, 5)], clouds(4, 2))


def test_lists_of_different_lengths_raise(metric):
    with pytest.raises(ValueError, match="3 partial clouds against 2 complete clouds"):
        metric.uhd_ragged(clouds(3, 5, 1), clouds(4, 2))
    with pytest.raises(ValueError, match="2 partial clouds against 1 complete clouds"):
        metric.uhd_ragged((torch.zeros(8, 3), [0, 3, 8]), clouds(4))


def test_an_element_that_is_not_n_by_3_raises(metric):
    with pytest.raises(ValueError, match=r"partials\[1\] must be an \[N,3\] tensor"):
        metric.uhd_ragged([torch.zeros(3, 3), torch.zeros(5, 2)], clouds(4, 2))
    with pytest.raises(ValueError, match=r"completes\[0\] must be an \[N,3\] tensor"):
        metric.uhd_ragged(clouds(3), [torch.zeros(2, 4, 3)])
    with pytest.raises(ValueError, match="packed partials must be"):
        metric.uhd_ragged((torch.zeros(8, 2), [0, 3, 8]), clouds(4, 2))
    with pytest.raises(ValueError, match="offsets of partials must ascend from 0 to its 8 points"):
        metric.uhd_ragged((torch.zeros(8, 3), [0, 3, 7]), clouds(4, 2))
    with pytest.raises(TypeError):
        metric.uhd_ragged(torch.zeros(2, 8, 3), clouds(4, 2))
    with pytest.raises(TypeError):
        metric.uhd_ragged([c.half() for c in clouds(3, 5)], clouds(4, 2))


def test_float64_that_float32_cannot_hold_raises(metric):
    bad = torch.full((8, 3), 0.1, dtype=torch.float64)             # 0.1 is not a float32
    ok = torch.full((5, 3), 0.5, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"partials\[1\] is float64 and not representable in float32"):
        metric.uhd_ragged([ok, bad], [ok, ok])
    with pytest.raises(ValueError, match=r"completes\[0\] is float64 and not representable in float32"):
        metric.uhd_ragged([ok, ok], [bad, ok])
    with pytest.raises(ValueError, match="float32"):
        metric.uhd_ragged((torch.cat([ok, bad]), [0, 5, 13]), [ok, ok])


def test_an_empty_cloud_raises_and_names_the_pair(metric):
    with pytest.raises(ValueError, match=r"pair 1 has an empty cloud \(N = 0, M = 2\)"):
        metric.uhd_ragged(clouds(3, 0, 4), clouds(4, 2, 1))
    with pytest.raises(ValueError, match=r"pair 2 has an empty cloud \(N = 4, M = 0\)"):
        metric.uhd_ragged(clouds(3, 1, 4), (torch.zeros(6, 3), [0, 4, 6, 6]))
    with pytest.raises(ValueError, match=r"pair 0 has an empty cloud \(N = 0, M = 0\)"):
        metric.uhd_ragged(clouds(0), clouds(0))


def test_ragged_items_program_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "uhd_ragged_table_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", CSRC, os.path.join(ROOT, "tests", "uhd_ragged_table_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "uhd_ragged_table_check: ok" in r.stdout, r.stdout


def test_ragged_items_header_needs_no_hip():
    text = open(os.path.join(CSRC, "ragged_items.h")).read()
    assert not re.search(r"#include\s*[<\"]hip|__global__|#include\s*\"common.h\"", text)
    assert re.findall(r"#include\s*(\S+)", text) == ['"ragged_table.h"']
