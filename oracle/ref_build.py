"""Recipe for oracle/_ref/: the reference's own Chamfer and EMD kernels, compiled for the CPU.

TEST INFRASTRUCTURE ONLY.  build() reads loss_functions/Chamfer3D/chamfer3D.cu and
loss_functions/emd/emd_cuda.cu from the reference checkout ($GENPC_REFERENCE, default
/root/reference), takes every ``__global__`` / ``__device__`` function out of them by its signature
and matching braces (never by line number), writes them unmodified to oracle/_ref/*.inc and compiles
them with oracle/ref_simt.h (CPU stand-in for the device environment) and oracle/ref_driver.cpp
(restated host code) into

    oracle/_ref/libgenpc_ref_m0.so   g++     -O2 -ffp-contract=off  -fno-fast-math   (arithmetic mode 0)
    oracle/_ref/libgenpc_ref_m1.so   ROCm's clang++ -O2 -ffp-contract=fast -mfma     (the contraction LLVM
                                     itself chooses for the reference's text)

No -march=native: the binaries travel to other machines.  oracle/_ref/ is ignored by git; nothing of
the reference's text and nothing compiled from it is ever committed.

Before compiling, every launch the driver restates (its REF_LAUNCH lines) is compared, in order, with
the ``kernel<<<grid, block>>>`` text of the reference; a difference fails the build.

Where the reference checkout is absent the recipe does nothing and leaves existing binaries alone.
"""
import os
import re
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(_HERE, "_ref")
SOURCES = {"chamfer": os.path.join("loss_functions", "Chamfer3D", "chamfer3D.cu"),
           "emd": os.path.join("loss_functions", "emd", "emd_cuda.cu")}
NAMESPACE = {"chamfer": "ref_chamfer", "emd": "ref_emd"}
LIBS = {0: os.path.join(OUT, "libgenpc_ref_m0.so"), 1: os.path.join(OUT, "libgenpc_ref_m1.so")}
_OWN = [os.path.join(_HERE, f) for f in ("ref_simt.h", "ref_driver.cpp", "ref_build.py")]


def reference_root():
    return os.environ.get("GENPC_REFERENCE", "/root/reference")


def reference_present():
    return all(os.path.isfile(os.path.join(reference_root(), p)) for p in SOURCES.values())


def _blank_comments_and_strings(text):
    """Same length as `text`, with comments and string / character literals replaced by blanks, so
    that brackets found in the result are code."""
    out = list(text)
    i, n = 0, len(text)
    while i < n:
        two = text[i:i + 2]
        if two == "//":
            j = text.find("\n", i)
            j = n if j < 0 else j
        elif two == "/*":
            j = text.find("*/", i + 2)
            j = n if j < 0 else j + 2
        elif text[i] in "\"'":
            q = text[i]
            j = i + 1
            while j < n and text[j] != q:
                j += 2 if text[j] == "\\" else 1
            j += 1
        else:
            i += 1
            continue
        for k in range(i, min(j, n)):
            if out[k] != "\n":
                out[k] = " "
        i = j
    return "".join(out)


def _match(code, start, open_ch, close_ch):
    """Index just past the bracket that closes code[start] (which must be open_ch)."""
    assert code[start] == open_ch
    depth = 0
    for k in range(start, len(code)):
        if code[k] == open_ch:
            depth += 1
        elif code[k] == close_ch:
            depth -= 1
            if depth == 0:
                return k + 1
    raise RuntimeError("unbalanced %s%s in the reference source" % (open_ch, close_ch))


def extract_device_functions(text):
    """[(name, source text)] of every __global__ / __device__ function, in file order."""
    code = _blank_comments_and_strings(text)
    found = []
    pos = 0
    for mt in re.finditer(r"__(?:global|device)__[^;{}()]*?\b(\w+)\s*\(", code):
        if mt.start() < pos:
            continue
        close = _match(code, mt.end() - 1, "(", ")")
        brace = code.find("{", close)
        if brace < 0 or code[close:brace].strip():
            continue                                   # a declaration, not a definition
        pos = _match(code, brace, "{", "}")
        found.append((mt.group(1), text[mt.start():pos]))
    return found


def _split_top_level(code):
    parts, depth, cur = [], 0, ""
    for ch in code:
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
        if ch == "," and depth == 0:
            parts.append(cur)
            cur = ""
        else:
            cur += ch
    parts.append(cur)
    return ["".join(p.split()) for p in parts]


def reference_launches(text):
    """[(kernel, grid, block)] of every `kernel<<<grid, block>>>` in file order, white space removed."""
    code = _blank_comments_and_strings(text)
    out = []
    for mt in re.finditer(r"(\w+)\s*<<<(.*?)>>>", code, re.S):
        cfg = _split_top_level(mt.group(2))
        if len(cfg) != 2:
            raise RuntimeError("launch of %s has %d configuration arguments; the stand-in knows "
                               "grid and block only" % (mt.group(1), len(cfg)))
        out.append((mt.group(1), cfg[0], cfg[1]))
    return out


def driver_launches(text):
    """{namespace: [(kernel, grid, block)]} of the driver's REF_LAUNCH lines, in file order."""
    code = _blank_comments_and_strings(text)
    out = {}
    for mt in re.finditer(r"^\s*REF_LAUNCH\s*\(", code, re.M):
        end = _match(code, mt.end() - 1, "(", ")")
        args = _split_top_level(code[mt.end():end - 1])
        ns, kernel = args[0].split("::")
        out.setdefault(ns, []).append((kernel, args[1], args[2]))
    return out


def check_launches(ref_texts, driver_text):
    mine = driver_launches(driver_text)
    for key, text in ref_texts.items():
        theirs = reference_launches(text)
        ours = mine.get(NAMESPACE[key], [])
        if theirs != ours:
            raise RuntimeError(
                "the launches oracle/ref_driver.cpp restates differ from %s:\n  reference: %r\n  driver:    %r"
                % (SOURCES[key], theirs, ours))


def rocm_clang():
    for root in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if root:
            p = os.path.join(root, "llvm", "bin", "clang++")
            if os.path.isfile(p):
                return p
    return shutil.which("clang++")


def _stale(target, deps):
    return (not os.path.exists(target)) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


def build(force=False, verbose=False):
    """-> {mode: path} of the binaries that exist afterwards."""
    if reference_present():
        ref_paths = {k: os.path.join(reference_root(), p) for k, p in SOURCES.items()}
        deps = _OWN + list(ref_paths.values())
        cxx = {0: shutil.which("g++") or shutil.which("c++"), 1: rocm_clang()}
        flags = {0: ["-ffp-contract=off", "-fno-fast-math"], 1: ["-ffp-contract=fast", "-fno-fast-math", "-mfma"]}
        todo = [m for m in (0, 1) if cxx[m] and (force or _stale(LIBS[m], deps))]
        if todo:
            os.makedirs(OUT, exist_ok=True)
            ref_texts = {}
            for key, path in ref_paths.items():
                with open(path, encoding="utf-8", errors="replace") as f:
                    ref_texts[key] = f.read()
            with open(os.path.join(_HERE, "ref_driver.cpp")) as f:
                check_launches(ref_texts, f.read())
            for key, text in ref_texts.items():
                funcs = extract_device_functions(text)
                if not funcs:
                    raise RuntimeError("no kernels found in %s" % ref_paths[key])
                with open(os.path.join(OUT, key + "_kernels.inc"), "w") as f:
                    f.write("\n\n".join(src for _, src in funcs) + "\n")
            for m in todo:
                cmd = [cxx[m], "-std=c++14", "-O2", "-fPIC", "-shared", "-fvisibility=hidden"] + flags[m] + [
                    "-DGENPC_REF_MODE=%d" % m, "-I", _HERE, os.path.join(_HERE, "ref_driver.cpp"),
                    "-o", LIBS[m] + ".tmp", "-lm"]
                if verbose:
                    print(" ".join(cmd))
                subprocess.check_call(cmd)
                os.replace(LIBS[m] + ".tmp", LIBS[m])
    return {m: p for m, p in LIBS.items() if os.path.exists(p)}


if __name__ == "__main__":
    print(build(force=True, verbose=True))
