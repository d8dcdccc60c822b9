"""The C-ABI library loads (no GPU needed) and exports every symbol that
include/genpc_hip.h declares; the ctypes table in genpc_amd/_lib.py lists exactly
those symbols with matching arity.  No compute call is made here."""
import os
import re

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def header_prototypes():
    txt = open(os.path.join(ROOT, "include", "genpc_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(?:int|float|const char \*)\s*(genpc_\w+)\s*\(([^)]*)\)\s*;", txt):
        args = m.group(2).strip()
        protos[m.group(1)] = 0 if args == "void" else len(args.split(","))
    return protos


def test_header_has_the_path():
    p = header_prototypes()
    for name in ("genpc_chamfer_forward", "genpc_chamfer_backward", "genpc_emd_forward", "genpc_emd_backward",
                 "genpc_nm_distance"):
        assert name in p
    assert p["genpc_emd_forward"] == 20        # b,n,m + 14 buffers + eps, iters + stream
    assert p["genpc_chamfer_forward"] == 10
    assert p["genpc_chamfer_backward"] == 12
    assert p["genpc_pose_loss_grad_batch"] == 17   # b, nc, v, vert_col, center, params, np, partial, partial_col, 3 weights, radius, size, 2 outputs + stream
    assert p["genpc_pose_loss_grad"] == 20         # (unchanged beside it: the single-element evaluation with the caller's neighbours)
    assert p["genpc_nn_plan"] == 6                 # b, n, m, ndir, cus, out
    assert p["genpc_hpr_plan"] == 5                # c, n, best_only, cus, out
    assert p["genpc_nn_seeded_step"] == 14         # b, nm, rest, center, params, ns, stat, posed, d1, i1, d2, i2, sample + stream


def test_library_exports_every_declared_symbol():
    from genpc_amd import build
    build.build(verbose=False)
    from genpc_amd import _lib
    protos = header_prototypes()
    assert set(protos) == set(_lib.SIGNATURES), set(protos) ^ set(_lib.SIGNATURES)
    for name, nargs in protos.items():
        fn = getattr(_lib.lib, name)           # AttributeError if not exported
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        assert fn is not None
    assert _lib.lib.genpc_abi_version() == _lib.ABI_VERSION
    assert _lib.ABI_VERSION == 28                  # genpc_hpr_plan added


def test_arith_mode_switch():
    from genpc_amd import _lib
    prev = _lib.lib.genpc_set_arith(0)
    assert _lib.lib.genpc_get_arith() == 0
    _lib.lib.genpc_set_arith(prev)
    assert _lib.lib.genpc_get_arith() == prev


def test_fps_tune_takes_0_or_256():
    """genpc_fps_tune (calling thread): 256 forces the multi-workgroup sampling, 0 the default choice, anything else is refused."""
    from genpc_amd import _lib
    L = _lib.lib
    prev = L.genpc_fps_tune(256)
    try:
        assert L.genpc_fps_tune(0) == 256
        assert L.genpc_fps_tune(1) == -1 and b"genpc_fps_tune" in L.genpc_last_error()
        assert L.genpc_fps_tune(0) == 0            # (a refused value leaves the setting as it was)
    finally:
        L.genpc_fps_tune(prev)


def test_cpu_tensors_are_rejected_loudly():
    import torch
    from genpc_amd.loss_functions import chamfer_3DDist, emdModule
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        chamfer_3DDist()(torch.zeros(1, 8, 3), torch.zeros(1, 8, 3))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        emdModule()(torch.zeros(1, 256, 3), torch.zeros(1, 256, 3), 0.005, 2)


def test_reference_api_names():
    import loss_functions
    from genpc_amd.utils.loss_util import Completionloss
    assert hasattr(loss_functions, "chamfer_3DDist") and hasattr(loss_functions, "emdModule")
    for m in ("chamfer_l1", "chamfer_l2", "chamfer_partial_l1", "chamfer_partial_l2", "emd_loss", "get_loss"):
        assert hasattr(Completionloss, m)
    with pytest.raises(Exception):
        Completionloss("nope")


def test_no_packed_fp32_instructions_in_the_shipped_code():
    """DESIGN.md 6a / tools/PACKED_FP32_OPSEL.md: packed fp32 arithmetic whose low lane selects a high half (op_sel) reads zeros
    in lanes 48-63 beside waves that interleave MFMA and vector instructions on this part, and the compiler emits such
    instructions wherever it pairs fp32 registers.  The library is built with the device feature off, and no source turns it
    back on for a function: every object is disassembled here and must hold no v_pk_*_f32 instruction, in any kernel."""
    import glob
    import subprocess
    import tempfile
    from genpc_amd import build
    for src in sorted(glob.glob(os.path.join(ROOT, "genpc_amd", "csrc", "*"))):
        with open(src, errors="replace") as f:
            assert "packed-fp32-ops" not in f.read(), src
    build.build(verbose=False)
    llvm = "/opt/rocm/lib/llvm/bin"
    objs = sorted(glob.glob(os.path.join(ROOT, "genpc_amd", "lib", "obj", "*.o")))
    assert objs, "no objects under genpc_amd/lib/obj"
    bad = []
    with tempfile.TemporaryDirectory() as tmp:
        for o in objs:
            fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
            subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", o, fat])
            if os.path.getsize(fat) == 0:
                continue
            targets = subprocess.check_output([llvm + "/clang-offload-bundler", "--list", "--type=o", "--input=" + fat], text=True).split()
            tgt = [t for t in targets if "gfx950" in t]
            assert tgt, (o, targets)
            subprocess.check_call([llvm + "/clang-offload-bundler", "--type=o", "--targets=" + tgt[0], "--input=" + fat, "--output=" + co, "--unbundle"])
            dis = subprocess.check_output([llvm + "/llvm-objdump", "-d", "--no-show-raw-insn", co], text=True)
            func = ""
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    func = m.group(1)
                elif re.search(r"\bv_pk_(add|mul|fma)_f32\b", line):
                    bad.append((os.path.basename(o), func, line.strip()))
    assert not bad, bad[:5]


# The library's tuning switches (environment variables read through genpc::tune_env / tune_env_str): only those that a test
# (tests/test_gpu_hpr_paths.py, tests/test_gpu_pose_update_forms.py) or a tool cited for its numbers (tools/nn_sweep.py,
# tools/prof_c2*.py) sets.  A switch nothing sets is a default written as code.
KEPT_SWITCHES = {
    "GENPC_HPR_SPLIT", "GENPC_HPR_NOCULL", "GENPC_HPR_HOME_TILES", "GENPC_HPR_HOME_CHUNKS", "GENPC_HPR_DECIDE_KERNEL",
    "GENPC_HPR_PARK_MB",
    "GENPC_POSE_DUAL", "GENPC_POSE_DUAL_FLAGS", "GENPC_POSE_FUSE_UPDATE", "GENPC_POSE_GRAD_RIDES", "GENPC_POSE_LOCKSTEP",
    "GENPC_POSE_SEEDED",
    "GENPC_NN_PATH", "GENPC_NN_Q", "GENPC_NN_U", "GENPC_NN_R", "GENPC_NN_WPS", "GENPC_NN_DEBUG",
}


def test_tuning_switches_are_the_kept_ones():
    """Every GENPC_* name the library passes to tune_env / tune_env_str is one of KEPT_SWITCHES and each of them is read; the
    Python package reads no GENPC_* variable from the environment but the library's path and the build's job count."""
    import glob
    found = set()
    for src in glob.glob(os.path.join(ROOT, "genpc_amd", "csrc", "*")):
        with open(src, errors="replace") as f:
            found |= set(re.findall(r"\btune_env(?:_str)?\s*\(\s*\"(GENPC_\w+)\"", f.read()))
    assert found == KEPT_SWITCHES, (sorted(found - KEPT_SWITCHES), sorted(KEPT_SWITCHES - found))
    py = set()
    for src in glob.glob(os.path.join(ROOT, "genpc_amd", "**", "*.py"), recursive=True):
        with open(src, errors="replace") as f:
            txt = f.read()
        py |= set(re.findall(r"\b(?:environ(?:\.get)?|getenv)\s*[\[(]\s*[\"'](GENPC_\w+)", txt))
    assert py == {"GENPC_LIB", "GENPC_BUILD_JOBS"}, sorted(py)
