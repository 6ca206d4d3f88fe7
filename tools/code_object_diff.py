#!/usr/bin/env python3
"""Compare the gfx950 machine code of two source trees, kernel by kernel, without a GPU.

usage: python tools/code_object_diff.py OLD NEW [--only REGEX] [--keep DIR] [-j N]

OLD and NEW are either source trees (a checkout of this repository, or its icka_amd/csrc directory) or directories of
code objects extracted earlier (``*.co``, as --keep leaves them).  For a source tree every ``.hip`` of icka_amd/csrc (--only:
those whose file name matches) is compiled with the Makefile's flags plus ``--offload-device-only`` and the gfx950 code
object is unbundled from the result.  For every kernel of a code object the tool reads
  * the kernel descriptor metadata of ``llvm-readelf --notes``: VGPR / AGPR / SGPR counts, spill counts, private segment,
    group segment and kernarg sizes;
  * the instruction text of ``llvm-objdump -d`` with addresses, encodings and symbol offsets removed.
Kernels are matched by demangled name across ALL units of a tree, so a kernel that moved to another file is still the same
kernel; ``(anonymous namespace)::`` is dropped from the names, so is one whose argument type left the unnamed namespace.
One line per kernel: identical | metadata differs | text differs (n lines) | missing | duplicate; exit status 1 unless every
kernel is identical.  The tool only compares: what the instructions are is none of its business."""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
          ".group_segment_fixed_size", ".kernarg_segment_size")


def run(cmd, **kw):
    return subprocess.run(cmd, check=True, capture_output=True, text=True, **kw).stdout


def makefile_flags(csrc):
    """FLAGS of the Makefile, as make expands them (ARCH and EXTRA at their defaults)."""
    db = run(["make", "-C", csrc, "-pn", "--no-print-directory"])
    flags = re.search(r"^FLAGS := (.*)$", db, re.M).group(1)
    hipcc = re.search(r"^HIPCC :?= (.*)$", db, re.M).group(1)
    return hipcc, flags.split()


def csrc_of(tree):
    for d in (os.path.join(tree, "icka_amd", "csrc"), tree):
        if os.path.isfile(os.path.join(d, "Makefile")) and any(f.endswith(".hip") for f in os.listdir(d)):
            return d
    return None


def build_objects(tree, out, only, jobs):
    """-> code object files of ``tree``: compiled into ``out`` from source, or the *.co files found in it."""
    csrc = csrc_of(tree)
    if csrc is None:
        cos = sorted(os.path.join(tree, f) for f in os.listdir(tree) if f.endswith(".co"))
        if not cos:
            sys.exit(f"{tree}: neither a source tree nor a directory of *.co code objects")
        return cos
    hipcc, flags = makefile_flags(csrc)
    units = sorted(f for f in os.listdir(csrc) if f.endswith(".hip") and (not only or re.search(only, f)))
    os.makedirs(out, exist_ok=True)

    def one(unit):
        dev = os.path.join(out, unit[:-4] + ".dev.o"), os.path.join(out, unit[:-4] + ".co")
        run([hipcc, *flags, "--offload-device-only", "-c", unit, "-o", dev[0]], cwd=csrc)
        run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={dev[0]}",
             f"--output={dev[1]}"])
        os.remove(dev[0])
        return dev[1]

    with ThreadPoolExecutor(jobs) as ex:
        return list(ex.map(one, units))


def demangle(names):
    out = run(["c++filt"], input="\n".join(names) + "\n").split("\n")
    return {n: d.replace("(anonymous namespace)::", "") for n, d in zip(names, out)}


def kernels_of(co):
    """-> {mangled kernel name: (metadata dict, [instruction lines])} of one code object."""
    notes = run([os.path.join(LLVM, "llvm-readelf"), "--notes", co])
    meta, cur = {}, None
    for ln in notes.split("\n"):
        if ln.startswith("  - "):            # a new entry of amdhsa.kernels
            cur = {}
            ln = "    " + ln[4:]
        m = re.match(r"^    (\.[a-z_]+): +(\S+)$", ln)
        if cur is not None and m:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == ".name":
                meta[m.group(2)] = cur
    # a function's text ends where its symbol does: what the assembler pads the gap to the next function with is not code
    size = {}
    for ln in run([os.path.join(LLVM, "llvm-readelf"), "-s", "--wide", co]).split("\n"):
        f = ln.split()
        if len(f) == 8 and f[3] == "FUNC":
            size[f[7]] = int(f[2])
    text, name, end = {}, None, 0
    for ln in run([os.path.join(LLVM, "llvm-objdump"), "-d", co]).split("\n"):
        m = re.match(r"^([0-9a-f]+) <(.+)>:$", ln)
        if m:
            name = m.group(2)
            end = int(m.group(1), 16) + size.get(name, 1 << 62)
            text[name] = []
        elif name and ln.startswith("\t"):
            at = re.search(r"// ([0-9A-F]+):", ln)
            if at and int(at.group(1), 16) < end:
                text[name].append(ln.split("//")[0].strip())
    return {k: ({f: v.get(f) for f in FIELDS}, text.get(k, [])) for k, v in meta.items()}


def tree_kernels(cos):
    found = {}   # demangled name -> [(unit, metadata, text)]
    for co in cos:
        ks = kernels_of(co)
        names = demangle(sorted(ks))
        for k, (m, t) in ks.items():
            found.setdefault(names[k], []).append((os.path.basename(co)[:-3], m, t))
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--only", help="regular expression on the .hip file names to compile (source trees)")
    ap.add_argument("--keep", help="directory that keeps the extracted code objects (DIR/old, DIR/new)")
    ap.add_argument("-j", type=int, default=4)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        base = a.keep or tmp
        old = tree_kernels(build_objects(a.old, os.path.join(base, "old"), a.only, a.j))
        new = tree_kernels(build_objects(a.new, os.path.join(base, "new"), a.only, a.j))
    bad = 0
    print(f"# {len(old)} kernels in OLD, {len(new)} in NEW; unit names are OLD -> NEW")
    for name in sorted(set(old) | set(new)):
        o, n = old.get(name, []), new.get(name, [])
        units = f"{'+'.join(u for u, _, _ in o) or '-'} -> {'+'.join(u for u, _, _ in n) or '-'}"
        if len(o) > 1 or len(n) > 1:
            verdict = "duplicate"
        elif not o or not n:
            verdict = "missing"
        elif o[0][1] != n[0][1]:
            verdict = "metadata differs (" + ", ".join(f"{f[1:]} {o[0][1][f]} -> {n[0][1][f]}" for f in FIELDS if o[0][1][f] != n[0][1][f]) + ")"
        elif o[0][2] != n[0][2]:
            d = [ln for ln in difflib.unified_diff(o[0][2], n[0][2], lineterm="", n=0) if ln[:1] in "+-" and ln[:3] not in ("+++", "---")]
            verdict = f"text differs ({len(d)} lines)"
        else:
            verdict = "identical"
        bad += verdict != "identical"
        print(f"{verdict:<24} {name}   [{units}]")
    print(f"# {bad} of {len(set(old) | set(new))} kernels not identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
