"""The host side of the ragged Chamfer distances, without a GPU: what chamfer_ragged refuses, how it packs, how the --clouds
CLI matches files, and csrc/ragged_table.h (offset validation, the pair table, the placements derived from it) as a
stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genpc_amd", "csrc")


@pytest.fixture(scope="module")
def ragged():
    from genpc_amd import build
    build.build(verbose=False)
    from genpc_amd.loss_functions.Chamfer3D import dist_chamfer_ragged
    return dist_chamfer_ragged


def clouds(*sizes):
    return [torch.arange(n * 3, dtype=torch.float32).reshape(n, 3) for n in sizes]


def test_cpu_tensors_raise(ragged):
    from genpc_amd import chamfer_3D
    from genpc_amd.metric import evaluate_clouds
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        ragged.chamfer_ragged(clouds(3, 5), clouds(4, 2))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        ragged.chamfer_ragged((torch.zeros(8, 3), [0, 3, 8]), (torch.zeros(6, 3), [0, 4, 6]))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        evaluate_clouds(clouds(3, 5), clouds(4, 2))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        chamfer_3D.nm_distance_ragged(torch.zeros(8, 3), [0, 3, 8], torch.zeros(6, 3), [0, 4, 6], torch.zeros(8),
                                      torch.zeros(8, dtype=torch.int32))


def test_length_and_shape_mismatches_raise(ragged):
    with pytest.raises(ValueError, match="3 clouds against 2"):
        ragged.chamfer_ragged(clouds(3, 5, 1), clouds(4, 2))
    with pytest.raises(ValueError, match="2 clouds against 1"):
        ragged.chamfer_ragged((torch.zeros(8, 3), [0, 3, 8]), clouds(4))
    with pytest.raises(ValueError, match=r"clouds1\[1\] must be an \[N,3\] tensor"):
        ragged.chamfer_ragged([torch.zeros(3, 3), torch.zeros(5, 2)], clouds(4, 2))
    with pytest.raises(ValueError, match=r"clouds2\[0\] must be an \[N,3\] tensor"):
        ragged.chamfer_ragged(clouds(3), [torch.zeros(2, 4, 3)])
    with pytest.raises(TypeError, match="float32"):
        ragged.chamfer_ragged(clouds(3), [torch.zeros(4, 3, dtype=torch.float64)])
    with pytest.raises(ValueError, match="packed clouds1 must be"):
        ragged.chamfer_ragged((torch.zeros(8, 2), [0, 3, 8]), clouds(4, 2))
    for off in ([0, 3, 7], [1, 3, 8], [0, 5, 3, 8], []):
        with pytest.raises(ValueError, match="offsets of clouds1 must ascend from 0 to its 8 points"):
            ragged.chamfer_ragged((torch.zeros(8, 3), off), clouds(4, 2))
    with pytest.raises(TypeError):
        ragged.chamfer_ragged(torch.zeros(2, 8, 3), clouds(4, 2))


def test_requires_grad_raises_and_names_the_differentiable_path(ragged):
    a = clouds(3, 5)
    a[1].requires_grad_(True)
    with pytest.raises(RuntimeError, match="chamfer_3DDist"):
        ragged.chamfer_ragged(a, clouds(4, 2))
    with pytest.raises(RuntimeError, match="chamfer_3DDist"):
        ragged.chamfer_ragged(clouds(4, 2), (torch.zeros(8, 3, requires_grad=True), [0, 3, 8]))


def test_packed_and_list_forms_give_the_same_offsets(ragged):
    cs = clouds(3, 0, 5, 1)
    points, off = ragged.pack_clouds(cs)
    assert off == [0, 3, 3, 8, 9] and tuple(points.shape) == (9, 3) and points.is_contiguous()
    assert torch.equal(points[3:8], cs[2])
    for given in (off, tuple(off), torch.tensor(off), torch.tensor(off, dtype=torch.int32)):
        p2, off2 = ragged.pack_clouds((points, given))
        assert off2 == off and all(type(v) is int for v in off2) and torch.equal(p2, points)
    assert ragged.pack_clouds([])[1] == [0]
    # a tuple of two clouds is a list of clouds, not (points, offsets)
    assert ragged.pack_clouds((torch.zeros(4, 3), torch.zeros(2, 3)))[1] == [0, 4, 6]


def test_offsets_reach_the_library_as_host_ints():
    from genpc_amd import chamfer_3D
    arr, lst = chamfer_3D._host_offsets(torch.tensor([0, 4, 9]), "noff")
    assert list(arr) == [0, 4, 9] and lst == [0, 4, 9]
    assert list(chamfer_3D._host_offsets((0, 2), "noff")[0]) == [0, 2]
    with pytest.raises(ValueError):
        chamfer_3D._host_offsets([0, 2 ** 31], "noff")
    with pytest.raises(ValueError):
        chamfer_3D._host_offsets([], "noff")
    with pytest.raises(TypeError):
        chamfer_3D._host_offsets(torch.tensor([0.0, 2.0]), "noff")


def test_clouds_cli_matches_files_by_name(tmp_path):
    from genpc_amd.metric import match_cloud_files
    pred, gt = tmp_path / "pred", tmp_path / "gt"
    pred.mkdir()
    gt.mkdir()
    for d, names in ((pred, ["b.ply", "a.ply", "only_pred.ply", "notes.txt", "c.PLY"]), (gt, ["a.ply", "b.ply", "only_gt.ply", "c.PLY"])):
        for n in names:
            (d / n).write_bytes(b"")
    (gt / "dir.ply").mkdir()
    pairs, only_pred, only_gt = match_cloud_files(str(pred), str(gt))
    assert [p[0] for p in pairs] == ["a.ply", "b.ply", "c.PLY"]
    assert all(p[1] == str(pred / p[0]) and p[2] == str(gt / p[0]) for p in pairs)
    assert only_pred == ["only_pred.ply"] and only_gt == ["only_gt.ply"]


def test_ragged_table_program_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "ragged_table_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", CSRC, os.path.join(ROOT, "tests", "ragged_table_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "ragged_table_check: ok" in r.stdout, r.stdout


def test_ragged_table_header_needs_no_hip():
    text = open(os.path.join(CSRC, "ragged_table.h")).read()
    assert "__global__" not in text
    assert re.findall(r"#include\s*(\S+)", text) == ['"ragged_offsets.h"']          # (plain C++ itself: tests/test_ragged_offsets.py)
