"""The host side of the ragged mesh sampler and of reg over a list of scans, without a GPU: genpc_mesh_sample_ragged is
declared, bound and exported and the ABI version stands; every refusal of the C entry point comes back as -1 with its message
before anything touches a device (null stream, dummy pointers: nothing is enqueued); csrc/mesh_sample_ragged_plan.h -- which
mesh a work item serves, where its chunk sums lie, how large the scratch is -- as a stand-alone program under the address and
undefined-behaviour sanitizers (tests/mesh_sample_ragged_plan_check.cpp; nothing loaded into Python is sanitized); and what
mesh_io.sample_surfaces_gpu, reg_xyz.reg_tensors_scans and reg_xyz.reg_scans refuse before any work."""
import ctypes
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_abi import header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genpc_amd", "csrc")
DUMMY = ctypes.c_void_p(0x1000)          # never dereferenced: every case below is decided on the host
NULL = ctypes.c_void_p(0)
PREFIX = "genpc_mesh_sample_ragged: "


@pytest.fixture(scope="module")
def L():
    from genpc_amd import build
    build.build(verbose=False)
    from genpc_amd import _lib
    return _lib


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def words(*v):
    return (ctypes.c_ulonglong * len(v))(*v)


def call(L, c, voff, foff, soff, seeds, vertices=DUMMY, colors=NULL, faces=DUMMY, out=DUMMY, out_colors=NULL, status=DUMMY):
    cast = lambda a: NULL if a is None else ctypes.cast(a, ctypes.c_void_p)
    return L.lib.genpc_mesh_sample_ragged(c, cast(voff), cast(foff), cast(soff), cast(seeds), vertices, colors, faces, out, out_colors,
                                          NULL, NULL, status, None)


def max_meshes():
    m = re.search(r"#define\s+GENPC_MESH_SAMPLE_RAGGED_MAX_MESHES\s+(\d+)", open(os.path.join(ROOT, "include", "genpc_hip.h")).read())
    assert m, "the header exports the bound as a constant"
    return int(m.group(1))


def test_declared_bound_and_exported(L):
    p = header_prototypes()
    # c, voff, foff, soff, seeds, vertices, vertex_colors, faces, out_xyz, out_colors, out_face, out_bary, out_status + stream
    assert p.get("genpc_mesh_sample_ragged") == 14
    assert len(L.SIGNATURES["genpc_mesh_sample_ragged"][1]) == 14
    assert set(p) == set(L.SIGNATURES)
    assert L.lib.genpc_mesh_sample_ragged is not None
    assert L.ABI_VERSION == 28 and L.lib.genpc_abi_version() == 28      # additive: the number stays
    from genpc_amd.utils import mesh_io
    assert mesh_io.MESH_SAMPLE_RAGGED_MAX_MESHES == max_meshes()
    plan = open(os.path.join(CSRC, "mesh_sample_ragged_plan.h")).read()
    assert re.search(r"kMsRaggedMaxMeshes\s*=\s*%d\b" % max_meshes(), plan)
    text = open(os.path.join(CSRC, "mesh_sample_ragged.hip")).read()
    assert re.search(r"ws_alloc\(L, kWsMeshSampleRagged, st\)", text)
    assert "kWsMeshSampleRagged = 48" in open(os.path.join(CSRC, "common.h")).read()


def test_refusals(L):
    n = max_meshes()
    up, sd = ints(0, 5, 9), words(1, 2)
    cases = [
        ("negative number of meshes", -1, up, up, up, sd),
        ("more than %d meshes" % n, n + 1, ints(*range(n + 2)), ints(*range(n + 2)), ints(*range(n + 2)), words(*range(n + 1))),
        ("null offset or seed table", 2, None, up, up, sd),
        ("null offset or seed table", 2, up, None, up, sd),
        ("null offset or seed table", 2, up, up, None, sd),
        ("null offset or seed table", 2, up, up, up, None),
        ("offsets must start at 0", 2, ints(1, 5, 9), up, up, sd),
        ("offsets must start at 0", 2, up, ints(1, 5, 9), up, sd),
        ("offsets must start at 0", 2, up, up, ints(1, 5, 9), sd),
        ("offsets must ascend", 2, ints(0, 9, 5), up, up, sd),
        ("offsets must ascend", 2, up, ints(0, 9, 5), up, sd),
        ("offsets must ascend", 2, up, up, ints(0, 9, 5), sd),
        ("every mesh needs 1 <= nf <= 2^24 faces", 2, up, ints(0, 5, 5), up, sd),
        ("every mesh needs 1 <= nf <= 2^24 faces", 2, up, ints(0, 0, 5), up, sd),
        ("every mesh needs 1 <= nf <= 2^24 faces", 1, ints(0, 5), ints(0, (1 << 24) + 1), ints(0, 5), sd),
        ("every mesh needs nv >= 1 vertices", 2, ints(0, 5, 5), up, up, sd),
        ("more than 2^28 vertices, faces or samples", 1, ints(0, (1 << 28) + 1), ints(0, 5), ints(0, 5), sd),
        ("more than 2^28 vertices, faces or samples", 1, ints(0, 5), ints(0, 5), ints(0, (1 << 28) + 1), sd),
    ]
    for msg, c, voff, foff, soff, seeds in cases:
        assert call(L, c, voff, foff, soff, seeds) == -1, msg
        err = L.last_error()
        assert err.startswith(PREFIX) and msg in err, (msg, err)


def test_null_pointers_and_colours_without_vertex_colours(L):
    up, sd = ints(0, 5, 9), words(1, 2)
    assert call(L, 2, up, up, up, sd, out_colors=DUMMY) == -1
    assert L.last_error() == PREFIX + "out_colors without vertex_colors"
    for kw in (dict(vertices=NULL), dict(faces=NULL), dict(out=NULL), dict(status=NULL)):
        assert call(L, 2, up, up, up, sd, **kw) == -1, kw
        assert L.last_error() == PREFIX + "null pointer", kw


def test_no_mesh_returns_1(L):
    assert call(L, 0, None, None, None, None, vertices=NULL, faces=NULL, out=NULL, status=NULL) == 1      # not even the tables are looked at


def test_the_limit_itself_is_not_refused_for_its_number(L):
    n = max_meshes()
    off = ints(*range(n + 1))
    assert call(L, n, off, off, off, words(*range(n)), vertices=NULL) == -1
    assert L.last_error() == PREFIX + "null pointer"


def test_plan_program_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "mesh_sample_ragged_plan_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", CSRC, os.path.join(ROOT, "tests", "mesh_sample_ragged_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "mesh_sample_ragged_plan_check: ok" in r.stdout, r.stdout


def test_plan_header_needs_no_hip():
    text = open(os.path.join(CSRC, "mesh_sample_ragged_plan.h")).read()
    assert not re.search(r"#include\s*[<\"]hip|__global__|#include\s*\"common.h\"", text)
    assert re.findall(r"#include\s*(\S+)", text) == ['"ragged_offsets.h"', '"ws_layout.h"']          # (the first: tests/test_ragged_offsets.py)


def mesh(nv=4, nf=2):
    V = np.arange(nv * 3, dtype=np.float32).reshape(nv, 3)
    F = np.zeros((nf, 3), np.int32)
    return V, F


def test_sample_surfaces_gpu_refuses(L):
    from genpc_amd.utils import mesh_io as M
    f = M.sample_surfaces_gpu
    V, F = mesh()
    with pytest.raises(RuntimeError, match=r"GPU tensors only .*meshes\[1\]"):
        f([(V, F), (torch.from_numpy(V), F)], 8, 0)
    with pytest.raises(ValueError, match="2 counts for 3 meshes"):
        f([(V, F)] * 3, [8, 8], 0)
    with pytest.raises(ValueError, match="2 seeds for 1 meshes"):
        f([(V, F)], 8, [0, 1])
    with pytest.raises(TypeError, match="seeds must be ints"):
        f([(V, F)], 8, 0.5)
    with pytest.raises(TypeError, match="seeds must be ints"):
        f([(V, F)], 8, [True])
    with pytest.raises(TypeError, match="counts must be ints"):
        f([(V, F)], 8.0, 0)
    with pytest.raises(ValueError, match="counts must be in"):
        f([(V, F)], -1, 0)
    with pytest.raises(ValueError, match="seeds must be in"):
        f([(V, F)], 8, 1 << 64)
    with pytest.raises(TypeError, match=r"meshes\[0\] must be"):
        f([V], 8, 0)
    with pytest.raises(TypeError, match="meshes is a list"):
        f(V, 8, 0)
    with pytest.raises(ValueError, match=r"meshes\[1\] needs vertices \[nv,3\] and faces \[nf,3\]"):
        f([(V, F), (V, F[:, :2])], 8, 0)
    with pytest.raises(ValueError, match=r"meshes\[0\] needs nv >= 1 and 1 <= nf"):
        f([(V, F[:0])], 8, 0)
    with pytest.raises(ValueError, match=r"colors of meshes\[0\]"):
        f([(V, F, V[:2])], 8, 0)
    assert f([], 8, 0) == [] and f([], [], []) == []


def clouds(*sizes):
    return [torch.arange(n * 3, dtype=torch.float32).reshape(n, 3) for n in sizes]


def test_reg_tensors_scans_refuses(L):
    from genpc_amd import reg_xyz
    f = reg_xyz.reg_tensors_scans
    assert f([], []) == []
    with pytest.raises(ValueError, match="2 partials against 1 completes"):
        f(clouds(5, 7), clouds(5))
    with pytest.raises(TypeError, match="lists of"):
        f(clouds(5)[0], clouds(5))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        f(clouds(5, 7), clouds(5, 7))
    with pytest.raises(ValueError, match=r"completes\[1\] must be an \[N,3\] tensor"):
        f(clouds(5, 7), [torch.zeros(5, 3), torch.zeros(5, 2)])
    with pytest.raises(ValueError, match="diff_transforms is None or a list of one entry per scan"):
        f(clouds(5, 7), clouds(5, 7), diff_transforms=[np.eye(4)])
    with pytest.raises(ValueError, match="partial_cols is None or a list"):
        f(clouds(5, 7), clouds(5, 7), partial_cols=clouds(5))


def test_reg_scans_refuses_before_any_work(tmp_path):
    from genpc_amd import reg_xyz
    cfg = SimpleNamespace(output_path=str(tmp_path), device="cuda", generative_model="trellis", dataset="redwood")
    for flag in ("a", "b"):
        os.makedirs(tmp_path / flag)
        open(tmp_path / flag / "color_point.ply", "w").close()
    open(tmp_path / "a" / "a_trellis.glb", "w").close()
    # flag b's mesh is missing: named before flag a's (empty, unreadable) files are opened
    with pytest.raises(FileNotFoundError, match=re.escape(str(tmp_path / "b" / "b_trellis.glb"))):
        reg_xyz.reg_scans(cfg, ["a", "b"], seed=7)
    with pytest.raises(TypeError, match=r"unexpected keyword argument\(s\) \['sead'\]"):
        reg_xyz.reg_scans(cfg, ["a", "b"], sead=7)
    with pytest.raises(TypeError, match="seed must be an int"):
        reg_xyz.reg_scans(cfg, ["a"], seed="7")
    with pytest.raises(TypeError, match="exclude"):
        reg_xyz.reg_scans(cfg, ["a"], seed=7, rng=np.random.default_rng(0))
    with pytest.raises(TypeError, match="flags is a list"):
        reg_xyz.reg_scans(cfg, "a", seed=7)
    assert reg_xyz.reg_scans(cfg, [], seed=7) == []
