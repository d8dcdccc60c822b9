"""What every ragged call shares, without a GPU: csrc/ragged_offsets.h (the offset check, the padded copy, the two searches) and
csrc/ragged_cand.h (the candidate table of the ICP and scale search calls) are plain C++ and are checked by a stand-alone program
under the address and undefined-behaviour sanitizers (tests/ragged_offsets_check.cpp; nothing loaded into Python is sanitized);
that each is stated once is checked as text; genpc_amd/_ragged.py's chunk generator is checked directly."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genpc_amd", "csrc")


def test_ragged_offsets_program_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "ragged_offsets_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-I", CSRC, os.path.join(ROOT, "tests", "ragged_offsets_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "ragged_offsets_check: ok" in r.stdout, r.stdout


def test_the_headers_need_no_hip():
    for name in ("ragged_offsets.h", "ragged_cand.h"):
        text = open(os.path.join(CSRC, name)).read()
        assert not re.search(r"#include\s*[<\"]hip|__global__|#include\s*\"(common|nn|grid)\.h\"", text), name


def test_each_piece_is_stated_once():
    texts = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip"))}
    code = {f: "\n".join(l.split("//")[0] for l in t.splitlines()) for f, t in texts.items()}
    for pattern, home in ((r"\(lo \+ hi \+ 1\) >> 1", "ragged_offsets.h"), (r"offsets must ascend", "ragged_offsets.h"),
                          (r"offsets must start at 0", "ragged_offsets.h"), (r"j < c \? j : c\]", "ragged_offsets.h"),
                          (r"int ragged_refuse\(const char \*fn, const char \*what\)\s*\{", "common.hip"),
                          (r"has candidates and an empty", "ragged_cand.h"), (r"__host__ __device__\s*$", "ragged_offsets.h")):
        found = [f for f, t in code.items() for _ in re.finditer(pattern, t, re.M)]
        assert found == [home], (pattern, found)


@pytest.mark.parametrize("tables", [1, 2, 3])
@pytest.mark.parametrize("entries", ["0", "1", "limit", "limit + 1", "2 * limit + 1"])
def test_chunks_tile_the_entries_and_rebase_the_tables(entries, tables):
    from genpc_amd._ragged import chunks
    limit = 5
    s = eval(entries, {"limit": limit})
    offs = [[0] for _ in range(tables)]
    for j in range(s):
        for t, off in enumerate(offs):
            off.append(off[-1] + (j * (t + 2) + t) % 4)          # (sizes 0 .. 3, empty entries among them, different per table)
    got = list(chunks(limit, *offs))
    assert len(got) == (s + limit - 1) // limit
    back = [[0] for _ in range(tables)]
    at = 0
    for item in got:
        a, b, rebased = item[0], item[1], item[2:]
        assert a == at and a < b <= s and b - a <= limit and len(rebased) == tables
        at = b
        for t in range(tables):
            assert isinstance(rebased[t], list) and len(rebased[t]) == b - a + 1 and rebased[t][0] == 0
            back[t] += [v + offs[t][a] for v in rebased[t][1:]]
    assert at == s and back == offs
