#!/usr/bin/env python3
"""Compare the gfx950 code of two builds, kernel by kernel, without a GPU.

usage: codeobj_diff.py OLD NEW [--allow KERNEL_SUBSTRING ...] [--by-name]      (OLD / NEW: a .so, a host .o, or a bare gfx950 code object)

Every gfx950 code object of the two files is disassembled (llvm-objdump -d --no-show-raw-insn), split per kernel symbol,
and compared instruction for instruction with addresses and `<symbol+off>` branch targets stripped; the four resource
figures of every kernel (llvm-readelf --notes) are compared too.  Kernels that differ are listed with their instruction
counts and the first differing line, every figure that moved as old -> new.  Exit status 1 on any difference;
--allow limits which kernels MAY differ in instructions or figures (their differences are still listed).
--by-name matches kernels by their demangled name and template arguments without the parameter list: for a change that renames
a parameter's type (the mangled symbol carries it) and nothing else about the kernel.
"""
import argparse, os, re, subprocess, sys, tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_store_hazard import LLVM, MAGIC, code_objects  # noqa: E402

FIGURES = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
SYM = re.compile(r"^[0-9a-f]+ <([^>]+)>:$")
KEY = re.compile(r"^(  - |    )(\.[a-z_]+):\s+(\S+)\s*$")
TARGET = re.compile(r"\s*<[^>]+>\s*$")


def kernels(path, tmp):
    """{"kernel symbol [code object i]": (instruction lines, {figure: value})} over every gfx950 code object of `path`."""
    os.makedirs(tmp)
    cos = code_objects(path, tmp) if MAGIC in open(path, "rb").read() else [path]
    out = {}
    for n, co in enumerate(cos):
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
        figs, cur = {}, None              # amdhsa.kernels: one "  - " entry per kernel, its own keys at that depth
        for ln in notes.splitlines():
            m = KEY.match(ln)
            if not m:
                continue
            if m.group(1) == "  - ":
                cur = {}
            if m.group(2) == ".name":
                figs[m.group(3).strip("'\"")] = cur
            elif m.group(2) in FIGURES:
                cur[m.group(2)] = int(m.group(3))
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
        sym = None
        for ln in dis.splitlines():
            m = SYM.match(ln.strip())
            if m:
                sym = "%s [code object %d]" % (m.group(1), n)
                if m.group(1) in figs:
                    out[sym] = ([], {k: figs[m.group(1)].get(k) for k in FIGURES})
                continue
            s = TARGET.sub("", ln.split("//")[0]).strip()
            if s and sym in out and not s.endswith(":"):
                out[sym][0].append(" ".join(s.split()))
    return out


def by_name(ks):
    """The same table keyed by "namespace::kernel<template arguments> [code object i]"."""
    syms = [k.split(" [")[0] for k in ks]
    names = subprocess.run(["c++filt"] + syms, check=True, capture_output=True, text=True).stdout.splitlines()
    out = {}
    for k, name in zip(ks, names):
        depth = 0
        for i, ch in enumerate(name):
            depth += (ch == "<") - (ch == ">")
            if ch == "(" and depth == 0 and i and name[i - 1] != "<":
                name = name[:i]
                break
        key = re.sub(r"^void ", "", name) + " [" + k.split(" [")[1]
        assert key not in out, key
        out[key] = ks[k]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--allow", action="append", default=[], metavar="KERNEL_SUBSTRING")
    ap.add_argument("--by-name", action="store_true")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old, new = kernels(a.old, os.path.join(tmp, "old")), kernels(a.new, os.path.join(tmp, "new"))
    if a.by_name:
        old, new = by_name(old), by_name(new)
    bad = 0
    for k in sorted(set(old) ^ set(new)):
        print("only in %s: %s" % ("OLD" if k in old else "NEW", k))
        bad += 1
    same = differ = moved = 0
    for k in sorted(set(old) & set(new)):
        (io, fo), (inn, fn) = old[k], new[k]
        allowed = any(s in k for s in a.allow)
        if io != inn:
            differ += 1
            bad += not allowed
            i = next((i for i, (x, y) in enumerate(zip(io, inn)) if x != y), min(len(io), len(inn)))
            print("differs%s: %s\n    instructions %d -> %d; first difference at %d:\n      - %s\n      + %s"
                  % (" (allowed)" if allowed else "", k, len(io), len(inn), i, io[i] if i < len(io) else "<end>", inn[i] if i < len(inn) else "<end>"))
        else:
            same += 1
        if fo != fn:
            moved += 1
            bad += not allowed
            print("figures%s: %s\n    %s" % (" (allowed)" if allowed else "", k, ", ".join("%s %s -> %s" % (f, fo[f], fn[f]) for f in FIGURES if fo[f] != fn[f])))
    print("%d kernels, %d instructions: %d identical, %d differ, %d with a resource figure that moved, %d not allowed"
          % (len(set(old) & set(new)), sum(len(v[0]) for v in new.values()), same, differ, moved, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
