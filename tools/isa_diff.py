#!/usr/bin/env python3
"""Kernel by kernel, is the machine code of two `hipcc -S --cuda-device-only` dumps the same text?
isa_diff.py <parent.s> <change.s> [--may-differ SUBSTRING]...   exit status 1 if a kernel outside the may-differ list differs.
Kernels only (symbols with an .amdhsa_kernel descriptor): a device function that was not inlined is not compared."""
import argparse
import difflib
import re
import sys


def kernels(path):
    """{kernel symbol: its lines from the entry label to .Lfunc_end (instructions, labels and the kernel descriptor with its register
    and scratch sizes), comments and blank space dropped}"""
    lines = open(path).read().split("\n")
    names = [m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))]
    out = {}
    for name in names:
        i = next(k for k, l in enumerate(lines) if l.startswith(name + ":")) + 1
        body = []
        while not lines[i].startswith(".Lfunc_end"):
            t = " ".join(lines[i].split(";")[0].split())
            if t:
                body.append(t)
            i += 1
        out[name] = body
    return out


def n_instructions(body):
    return sum(1 for t in body if not t.startswith(".") and not t.endswith(":"))


ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("parent")
ap.add_argument("change")
ap.add_argument("--may-differ", action="append", default=[], metavar="SUBSTRING")
args = ap.parse_args()
a, b = kernels(args.parent), kernels(args.change)
bad = 0
for name in sorted(set(a) | set(b)):
    allowed = any(s in name for s in args.may_differ)
    if name not in a or name not in b:
        verdict = "only in " + (args.parent if name in a else args.change)
    elif a[name] == b[name]:
        print("identical      ", name)
        continue
    else:
        ops = difflib.SequenceMatcher(None, a[name], b[name], autojunk=False).get_opcodes()
        changed = sum((i2 - i1) + (j2 - j1) for op, i1, i2, j1, j2 in ops if op != "equal")
        verdict = f"instructions {n_instructions(a[name])} -> {n_instructions(b[name])}, {changed} differing lines"
    bad += not allowed
    print("differs (ok)   " if allowed else "DIFFERS        ", name, "--", verdict)
print(f"{len(a)} / {len(b)} kernels, {bad} differ outside the may-differ list")
sys.exit(1 if bad else 0)
