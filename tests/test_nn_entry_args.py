"""The four kernels that take NNArgs (nn_f16_kernel, nn_finish_kernel, nn_mfma_kernel, nn_forward_kernel) read their kernel
arguments in ONE round of scalar loads at entry and decode the block id without a runtime division (csrc/nn.h NN_ARG / NN_HELD /
NN_OF_DIR, csrc/nn_decode.h).  No GPU: the built objects are disassembled, as tests/test_abi.py does for the packed-fp32 check, and the
decode header is compared with / and % by a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "genpc_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = {"nn_f16_kernel": 20, "nn_finish_kernel": 4, "nn_mfma_kernel": 8, "nn_forward_kernel": 4}     # instantiations

VMEM = re.compile(r"^(global|flat|buffer)_")
SREG = re.compile(r"^s(\d+)$|^s\[(\d+):(\d+)\]$")


def _sregs(operand):
    m = SREG.match(operand)
    if not m:
        return range(0)
    return range(int(m.group(1)), int(m.group(1)) + 1) if m.group(1) else range(int(m.group(2)), int(m.group(3)) + 1)


def disassemble(obj, tmp):
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
    targets = subprocess.check_output([LLVM + "/clang-offload-bundler", "--list", "--type=o", "--input=" + fat], text=True).split()
    tgt = [t for t in targets if "gfx950" in t]
    assert tgt, (obj, targets)
    subprocess.check_call([LLVM + "/clang-offload-bundler", "--type=o", "--targets=" + tgt[0], "--input=" + fat, "--output=" + co, "--unbundle"])
    return subprocess.check_output([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", co], text=True)


def functions(dis):
    """name -> list of (mnemonic, [operands]) in address order"""
    out, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        text = line.split("//")[0].strip()
        if cur is None or not text:
            continue
        parts = text.split(None, 1)
        cur.append((parts[0], [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []))
    return out


def entry_facts(code):
    """What stands between a kernel's entry and its first vector-memory instruction, and what the kernel-argument pointer
    s[0:1] is used for.  The pointer is followed until an instruction writes s0 or s1."""
    f = {"lgkm_waits": 0, "rcp_iflag": 0, "karg_loads": 0, "karg_reg_offset": 0, "karg_after_vmem": 0, "karg_after_first_wait": 0, "has_vmem": False}
    karg_alive, waited = True, False
    for op, args in code:
        if VMEM.match(op):
            f["has_vmem"] = True
        if op == "s_waitcnt":
            waited = True
        if not f["has_vmem"]:
            if op == "s_waitcnt" and any("lgkmcnt" in a for a in " ".join(args).split()):
                f["lgkm_waits"] += 1
            if op.startswith("v_rcp_iflag_f32"):
                f["rcp_iflag"] += 1
        if karg_alive and op.startswith("s_load_") and len(args) >= 3 and args[1] == "s[0:1]":
            f["karg_loads"] += 1
            if not re.match(r"^(0x[0-9a-f]+|\d+)$", args[2]) or len(args) > 3:
                f["karg_reg_offset"] += 1
            if f["has_vmem"]:
                f["karg_after_vmem"] += 1
            if waited:
                f["karg_after_first_wait"] += 1      # requested at entry means: before the first s_waitcnt of any kind
        # an instruction that writes s0 / s1 ends the pointer's life (its destination is its first operand; compares,
        # branches, waits and stores have none)
        if karg_alive and args and op.startswith("s_") and not re.match(r"s_(cmp|cmpk|bitcmp|cbranch|branch|waitcnt|barrier|nop|endpgm)", op):
            if any(r in (0, 1) for r in _sregs(args[0])):
                karg_alive = False
    return f


def kernel_facts():
    from genpc_amd import build
    build.build(verbose=False)
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("nn_f16", "nn_finish", "chamfer"):
            dis = disassemble(os.path.join(ROOT, "genpc_amd", "lib", "obj", name + ".o"), tmp)
            for fn, code in functions(dis).items():
                for k in KERNELS:
                    if re.match(r"_ZN5genpc\d+%sI" % k, fn):
                        found[fn] = (k, entry_facts(code))
    return found


needs_tools = pytest.mark.skipif(not (os.path.exists(LLVM + "/llvm-objdump") and os.path.exists(LLVM + "/clang-offload-bundler") and shutil.which("objcopy")),
                                 reason="no disassembler")


@needs_tools
def test_one_round_of_kernel_arguments_and_no_division_before_the_first_load():
    found = kernel_facts()
    count = {k: sum(1 for kk, _ in found.values() if kk == k) for k in KERNELS}
    assert count == KERNELS, count
    bad = []
    for fn, (k, f) in sorted(found.items()):
        assert f["has_vmem"] and f["karg_loads"] > 0, (fn, f)
        if f["lgkm_waits"] != 1 or f["karg_reg_offset"] or f["karg_after_vmem"] or f["karg_after_first_wait"] or f["rcp_iflag"]:
            bad.append((fn, f))
    assert not bad, bad[:4]


def test_entry_facts_on_a_listing():
    """The checker itself, on a few lines in the disassembler's format: a register offset, a second wait, a division and a late
    argument load are each seen; a load through s[0:1] after the pair was overwritten is not an argument load."""
    text = """
0000000000001000 <_ZN5genpc13nn_f16_kernelILi4ELi4ELi1ELi1ELi2048ELi8EEEvNS_6NNArgsE>:
	s_load_dword s3, s[0:1], 0xe0
	s_waitcnt lgkmcnt(0)
	s_mulk_i32 s3, 0x70
	s_load_dwordx4 s[4:7], s[0:1], s3 offset:0x60
	s_waitcnt lgkmcnt(0)
	v_rcp_iflag_f32_e32 v1, v1
	global_load_dword v2, v3, s[4:5]
	s_load_dword s8, s[0:1], 0x104
	s_mov_b64 s[0:1], s[6:7]
	s_load_dword s9, s[0:1], 0x0
	s_waitcnt vmcnt(0) lgkmcnt(0)
	s_endpgm
"""
    code = functions(text)["_ZN5genpc13nn_f16_kernelILi4ELi4ELi1ELi1ELi2048ELi8EEEvNS_6NNArgsE"]
    f = entry_facts(code)
    assert f == {"lgkm_waits": 2, "rcp_iflag": 1, "karg_loads": 3, "karg_reg_offset": 1, "karg_after_vmem": 1, "karg_after_first_wait": 2, "has_vmem": True}, f


@pytest.fixture(scope="module")
def decode_program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("nn_decode") / "nn_decode_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", CSRC, os.path.join(ROOT, "tests", "nn_decode_check.cpp"), "-o", exe], check=True)
    return exe


def test_nn_decode_program_under_sanitizers(decode_program):
    r = subprocess.run([decode_program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "nn_decode_check: ok" in r.stdout, r.stdout[-2000:]
    m = re.search(r"(\d+) rows of the plan table: (\d+) decoded block by block, (\d+) cell search, (\d+) nothing to do, (\d+) too large", r.stdout)
    assert m, r.stdout[-2000:]
    rows, decoded, grid, nothing, too_large = map(int, m.groups())
    assert rows == len(_table_asks("nn_plan_check.cpp", "kTable")) and decoded + grid + nothing + too_large == rows
    # the rows that launch none of the four kernels: two radius-limited calls and GENPC_NN_PATH -> 4, the empty ask, two that are too large
    assert (grid, nothing, too_large) == (3, 1, 2), m.group(0)


def _table_asks(name, array):
    """[(label, ask literal with its blanks squeezed)] of the rows of `array` in tests/<name>: the label and the first braced
    literal behind it."""
    src = open(os.path.join(ROOT, "tests", name)).read()
    body = src[src.index("%s[] = {" % array):]
    body = body[:body.index("\n};")]
    return [(label, re.sub(r"\s+", " ", ask)) for label, ask in re.findall(r'\{("(?:[^"\\]|\\.)*"),\s*(\{(?:[^{}]|\{[^{}]*\})*\})', body)]


def test_decode_check_repeats_every_row_of_the_plan_table():
    """tests/nn_plan_check.cpp may not be included (it has a main of its own): the decode check repeats its asks as literals, and
    this keeps the two lists the same, label by label and number by number."""
    table = _table_asks("nn_plan_check.cpp", "kTable")
    assert len(table) >= 70
    assert _table_asks("nn_decode_check.cpp", "kTableAsks") == table


def test_decode_header_is_shared():
    """One statement of the decode: the four kernels and the host call nn_decode.h, which holds no plan and no HIP include, and
    nn_plan.h stays free of device code."""
    text = open(os.path.join(CSRC, "nn_decode.h")).read()
    assert re.findall(r"#include\s*(\S+)", text) == ['"nn_plan.h"']
    assert "__device__" not in open(os.path.join(CSRC, "nn_plan.h")).read()
    srcs = {n: open(os.path.join(CSRC, n)).read() for n in ("chamfer.hip", "nn_f16.hip", "nn_finish.hip")}
    assert srcs["chamfer.hip"].count("nn_decode_block(") == 2 and srcs["nn_f16.hip"].count("nn_decode_block(") == 1
    assert srcs["nn_finish.hip"].count("nn_decode_fin(") == 1
    for n, s in srcs.items():
        code = "\n".join(l.split("//")[0] for l in s.splitlines())
        assert not re.search(r"%\s*(D\.|a\.|qblocks|fblocks|nbatch|hint_stride)", code), n
