"""The plan of an alignment call and of a silhouette step (csrc/pose_plan.h): which launches there are, on how many streams, how
they hand over, how wide they are.  No GPU: the header is plain C++ and is checked by a stand-alone program, a table of asks
with the plans they must give, under the address and undefined-behaviour sanitizers; that the loop decides nothing besides is
checked as text."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genpc_amd", "csrc")


def test_pose_plan_program_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "pose_plan_check")
    # (the sanitizers' runtimes linked statically -- clang's default, g++'s on request -- so that the program is checked the
    # same way whatever else the process environment loads beside it)
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", CSRC, os.path.join(ROOT, "tests", "pose_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0 and "pose_plan_check: ok" in r.stdout, r.stdout


def test_pose_plan_header_needs_no_hip():
    text = open(os.path.join(CSRC, "pose_plan.h")).read()
    assert not re.search(r"#include\s*[<\"]hip|__device__|__global__|#include\s*\"common.h\"", text)
    assert re.findall(r"#include\s*(\S+)", text) == ["<algorithm>"]


def _body(text, head):
    """The text of the function whose definition starts at `head`, braces matched."""
    i = text.index(head)
    j = text.index("{", text.index(")", i))
    depth, k = 0, j
    while True:
        depth += {"{": 1, "}": -1}.get(text[k], 0)
        k += 1
        if depth == 0:
            return text[j:k]


def test_the_loop_and_the_step_read_their_plans():
    """genpc_pose_optimize_batch and mask_step take their shape from pose_plan.h: the switches and the thread's modes go into
    the ask and are read nowhere else in the function, and the names of the decisions appear only as fields of the plan."""
    pose = open(os.path.join(CSRC, "pose.hip")).read()
    loop = _body(pose, "GENPC_API int genpc_pose_optimize_batch(")
    assert "pose_loop_plan(ask)" in loop
    for name in ("env_lock", "env_seeded", "env_dual0", "env_fuse_upd", "env_dual_flags", "env_ride", "serialised", "t_pose_dual", "t_pose_seeded"):
        uses = [l for l in loop.splitlines() if re.search(r"\b%s\b" % name, l)]
        assert uses and all("static const" in l or "ask." in l for l in uses), (name, uses)
    for name in ("lock", "dual", "flags", "fuse_upd", "ride", "seed_mode", "g_t", "g_g"):
        for l in loop.splitlines():
            code = l.split("//")[0]
            assert not re.search(r"(?<![\w.])%s\b" % name, code), (name, l)
    step = _body(open(os.path.join(CSRC, "mask_loss.hip")).read(), "int mask_step(")
    assert "mask_step_plan(" in step
    for name in ("gs", "gp", "fuse_w", "sub8"):
        for l in step.splitlines():
            assert not re.search(r"(?<![\w.])%s\b" % name, l.split("//")[0]), (name, l)


def test_each_kernel_is_defined_in_one_file():
    """Every file is compiled by itself: a kernel of the alignment loop lives in exactly one of its three, the shared device code
    in the two headers."""
    seen = {}
    for f in ("pose.hip", "mask_render.hip", "mask_loss.hip", "pose.h", "mask.h"):
        text = open(os.path.join(CSRC, f)).read()
        for m in re.finditer(r"__global__\s+(?:__launch_bounds__\([^)]*\)\s*)?void\s+(\w+)\s*\(", text):
            assert m.group(1) not in seen, (m.group(1), f, seen[m.group(1)])
            seen[m.group(1)] = f
    assert len(seen) == 21, sorted(seen)          # (29 kernels in the objects: mask_splat_kernel has two instances, mask_grad_kernel eight)
    assert not [k for k, f in seen.items() if f.endswith(".h")], seen
