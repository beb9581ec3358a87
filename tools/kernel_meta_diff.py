#!/usr/bin/env python3
"""Per-kernel metadata of two builds of libofdm_hip.so, side by side (the comparison DESIGN.md
section 6 describes): vgpr_count, vgpr_spill_count, sgpr_spill_count and group_segment_fixed_size of
every kernel, from `llvm-readelf --notes` on the library's gfx950 code objects.

    tools/kernel_meta_diff.py PARENT.so THIS.so > profiles/<name>_kernel_audit.txt

Kernels of PARENT.so are compared by name; kernels only in THIS.so are listed with their figures.
Needs no GPU.  Exit status 1 if a kernel of the parent build differs or is missing.

    tools/kernel_meta_diff.py --text PARENT.so THIS.so

compares the kernels' machine code as well (`llvm-objdump -d`, per kernel name, so the order of
instantiation inside a translation unit may move) and counts them per kernel family: the audit of a
change that must not touch device code.
"""
import argparse
import os
import re
import struct
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")
LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def code_objects(path, arch="gfx950"):
    """The device code objects for `arch` of every offload bundle in the file."""
    data = open(path, "rb").read()
    pos = data.find(MAGIC)
    while pos >= 0:
        (count,) = struct.unpack_from("<Q", data, pos + len(MAGIC))
        q = pos + len(MAGIC) + 8
        for _ in range(count):
            off, size, tlen = struct.unpack_from("<QQQ", data, q)
            triple = data[q + 24:q + 24 + tlen].decode()
            q += 24 + tlen
            if arch in triple and size:
                yield data[pos + off:pos + off + size]
        pos = data.find(MAGIC, pos + 1)


def short(demangled):
    """A kernel's name without return type, namespaces in front and parameter list."""
    return re.sub(r"^(void )?((\(anonymous namespace\)|ofdm)::)*|\(.*\)$", "", demangled)


def kernels(path):
    """{demangled kernel name: (the four FIELDS)} of a library."""
    out = {}
    for co in code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f.name], check=True,
                                   capture_output=True, text=True).stdout
        for block in re.split(r"\n  - ", notes):
            name = re.search(r"\.name:\s+(\S+)", block)
            vals = [re.search(r"\.%s:\s+(\d+)" % k, block) for k in FIELDS]
            if name and all(vals):
                out[name.group(1).strip("'\"")] = tuple(int(v.group(1)) for v in vals)
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), check=True,
                         capture_output=True, text=True).stdout.split("\n")
    return {short(d): out[n] for n, d in zip(names, dem)}


def texts(path):
    """{demangled kernel name: its disassembly, encodings included, addresses dropped} of a library."""
    out = {}
    for co in code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", f.name], check=True,
                                 capture_output=True, text=True).stdout
        for part in re.split(r"\n(?=[0-9a-f]{8,} <)", dis):
            head = re.match(r"[0-9a-f]+ <(\S+)>:\n", part)
            if head:
                # (a trailing "..." is the zero fill up to the next symbol's alignment: it belongs to the
                # order of the kernels in the object, not to the kernel)
                body = re.sub(r"\n\s*\.\.\.\s*$", "\n", part[head.end():].rstrip() + "\n")
                out[head.group(1)] = re.sub(r"// [0-9A-F]+:", "//", body)
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), check=True,
                         capture_output=True, text=True).stdout.split("\n")
    return {short(d): out[n] for n, d in zip(names, dem)}


def text_audit(parent, this, names):
    """Per-family counts and the kernels (`names`: those with metadata) whose machine code differs."""
    old, new = texts(parent), texts(this)
    fam = {}
    for k in names:
        fam[k.split("<")[0]] = fam.get(k.split("<")[0], 0) + 1
    diff = [k for k in names if k not in old or old[k] != new.get(k)]
    print(f"# machine code (llvm-objdump -d, per kernel name) of the parent's {len(names)} kernels, per family:\n# "
          + ", ".join(f"{f} {n}" for f, n in sorted(fam.items(), key=lambda x: -x[1])))
    print(f"# with different machine code in this build: {len(diff)}")
    for k in diff:
        print("# DIFFERENT TEXT:", k)
    return diff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text", action="store_true", help="compare the kernels' disassembly too")
    ap.add_argument("parent")
    ap.add_argument("this")
    a = ap.parse_args()
    old, new = kernels(a.parent), kernels(a.this)
    families = ("k_tx", "k_rx", "k_rx_prof", "k_rx_frames", "k_rx_dens", "k_rx_sweep", "k_rx_sweep_frames")
    fused = [k for k in old if k.startswith(tuple(f + "<" for f in families))]
    other = [k for k in old if k not in fused]
    diff_f = [k for k in fused if new.get(k) != old[k]]
    diff_o = [k for k in other if new.get(k) != old[k]]
    print("# Kernel metadata of libofdm_hip.so (llvm-readelf --notes on its gfx950 code objects), parent commit "
          "against this\n# commit: " + ", ".join(FIELDS) + " per kernel.")
    counts = ", ".join(f"{f} {sum(k.startswith(f + '<') for k in fused)}" for f in families)
    print(f"# fused kernels of the parent build: {len(fused)} ({counts}); with different figures in this build: "
          f"{len(diff_f)}")
    print(f"# other kernels of the parent build: {len(other)}, different: {len(diff_o)}")
    for k in diff_f + diff_o:
        print("# DIFFERENT:", k, old[k], "->", new.get(k))
    print("# new kernels: name  " + "  ".join(FIELDS))
    for k in sorted(set(new) - set(old)):
        print(k, *new[k])
    diff_t = text_audit(a.parent, a.this, sorted(old)) if a.text else []
    word = lambda n: str(n) if n else "none"
    print(f"# {word(len(set(diff_f + diff_o + diff_t)))} different, {word(len(set(new) - set(old)))} new, "
          f"{word(len(set(old) - set(new)))} missing")
    return 1 if diff_f or diff_o or diff_t else 0


if __name__ == "__main__":
    sys.exit(main())
