"""The plan of a ragged alignment call (csrc/pose_ragged_plan.h), without a GPU: the header is plain C++ and is checked by a
stand-alone program under the address and undefined-behaviour sanitizers (tests/pose_ragged_plan_check.cpp; nothing loaded into
Python is sanitized); that the entry points read it and decide nothing besides, and that the kernels state "where an element's
points lie" once, is checked as text."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genpc_amd", "csrc")

FIELDS = ("elements", "nc_max", "np_max", "total_c", "total_p", "replicate", "too_large", "g_t", "g_g", "gb", "g_m", "g_rep", "ride",
          "step", "nmax_piece", "blocks_per_cu", "fuse_w", "sub8", "gp", "gs")


def test_pose_ragged_plan_program_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "pose_ragged_plan_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", CSRC, os.path.join(ROOT, "tests", "pose_ragged_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "pose_ragged_plan_check: ok" in r.stdout, r.stdout


def test_pose_ragged_plan_header_needs_no_hip():
    text = open(os.path.join(CSRC, "pose_ragged_plan.h")).read()
    assert not re.search(r"#include\s*[<\"]hip|__device__|__global__|#include\s*\"(common|nn|grid|pose|mask)\.h\"", text)
    assert re.findall(r"#include\s*(\S+)", text) == ['"pose_plan.h"', '"ragged_table.h"']


def _body(text, head):
    """The text of the function that starts with `head`, braces matched."""
    i = text.index(head)
    j = text.index("{", text.index(")", i))
    depth, k = 0, j
    while True:
        depth += {"{": 1, "}": -1}.get(text[k], 0)
        k += 1
        if depth == 0:
            return text[j:k]


def test_the_entry_points_read_the_plan():
    """The three entry points take their shape from pose_ragged_plan.h: each asks pose_ragged_plan( once and names a decision only
    as a field of the plan; the launches they share do the same, and none of them waits for another kernel."""
    pose = open(os.path.join(CSRC, "pose.hip")).read()
    bodies = [_body(pose, "GENPC_API int %s(" % fn) for fn in ("genpc_pose_optimize_ragged", "genpc_pose_loss_grad_ragged", "genpc_pose_ragged_plan")]
    for body in bodies:
        assert len(re.findall(r"\bpose_ragged_plan\(ask\)", body)) == 1
    bodies += [_body(pose, "static int pose_ragged_step("), _body(pose, "static void pose_ragged_transform(")]
    for body in bodies:
        code = "\n".join(l.split("//")[0] for l in body.splitlines())
        for name in FIELDS:
            assert not re.search(r"(?<![\w.])%s\b" % name, code), (name, [l for l in code.splitlines() if re.search(r"(?<![\w.])%s\b" % name, l)][:2])
        for word in ("lin_grid(", "mask_step_plan(", "pose_loop_plan(", "PoseHandOver", "pose_side_of", "hipStreamWaitEvent", "hipEventRecord",
                     "hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy(", "nn_forward(", "launch_nn_seeded", "launch_nn_dedupe"):
            assert word not in code, word
    loop = _body(pose, "GENPC_API int genpc_pose_optimize_ragged(")
    assert "pose_pick_kernel" in loop and "pose_update_kernel" in loop and "PoseFuse" not in loop          # the update is a launch of its own
    # the existing loop is passed "no table": its body does not name one
    batch = _body(pose, "GENPC_API int genpc_pose_optimize_batch(")
    assert "coff" not in batch and "poff" not in batch and "pose_ragged" not in batch


def test_an_element_s_span_is_stated_once():
    """'Element e, n points at e * n' / 'off[e + 1] - off[e] points at off[e]' is pose.h's pose_span and nothing else: every
    per-point kernel of the loop calls it, and none multiplies an element number by a point count itself."""
    text = {f: open(os.path.join(CSRC, f)).read() for f in ("pose.h", "pose.hip", "mask_render.hip", "mask_loss.hip")}
    assert len(re.findall(r"PoseSpan pose_span\(", text["pose.h"])) == 1
    callers = {"pose.hip": ("pose_transform_kernel", "pose_transform_project_kernel", "pose_update_kernel", "mean3_accum_kernel", "mean3_finish_kernel"),
               "mask_render.hip": ("mask_project_kernel", "mask_splat_kernel"), "mask_loss.hip": ("mask_grad_kernel",), "pose.h": ("pose_grad_body",)}
    for f, names in callers.items():
        for name in names:
            assert "pose_span(" in _body(text[f], "void %s(" % name), (f, name)
    for f, t in text.items():
        code = "\n".join(l.split("//")[0] for l in t.splitlines())
        assert not re.search(r"\(size_t\)e \* (n|nc|np)\b", code.replace("PoseSpan{(size_t)e * n, n}", "")), f
    # the new kernels live in a file of their own, and there are two of them
    ragged = open(os.path.join(CSRC, "pose_ragged.hip")).read()
    assert sorted(re.findall(r"__global__\s+(?:__launch_bounds__\([^)]*\)\s*)?void\s+(\w+)\s*\(", ragged)) == \
        ["pose_ragged_replicate_kernel", "pose_ragged_tables_kernel"]
    assert "pose_wait_count" not in ragged and "s_sleep" not in ragged          # no spin


def test_the_search_is_split_behind_nn_h():
    nn_h = open(os.path.join(CSRC, "nn.h")).read()
    for decl in ("void nn_ragged_grids_layout(", "int nn_ragged_build(", "int nn_ragged_search("):
        assert decl in nn_h, decl
    rag = open(os.path.join(CSRC, "nn_ragged.hip")).read()
    whole = _body(rag, "static int nn_ragged(")
    assert "nn_ragged_build(" in whole and "nn_ragged_search(" in whole and "hipLaunchKernelGGL" not in whole
    common = open(os.path.join(CSRC, "common.h")).read()
    for slot in ("kWsPoseRaggedLoop = 49", "kWsPoseRaggedStep = 50", "kWsPoseRaggedReplicas = 51", "kWsPoseRaggedGridPartial = 52", "kWsPoseRaggedGridPosed = 53"):
        assert slot in common, slot
