#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of one source file, instruction for instruction.

    hipcc --offload-arch=gfx950 <csrc/Makefile's CXXFLAGS> -S --cuda-device-only -Rpass-analysis=kernel-resource-usage \
        -o NAME.s csrc/NAME.hip 2> NAME.remarks            # once at each commit
    tools/isa_compare.py before/NAME.s after/NAME.s [...]  # NAME.remarks is read from beside each NAME.s

A kernel is matched by its demangled name without the parameter list, so a kernel whose arguments changed still meets its
predecessor.  Compared: the text between the kernel's label and its .Lfunc_end with comments dropped, local labels renumbered
and the kernel's own symbol replaced; the kernel descriptor but for the kernarg size; and the compiler's resource remarks
(registers, scratch, LDS, occupancy).  Prints one line per file and one per kernel that differs; exits 1 if any does."""
import os
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {m: re.sub(r"^void |\((?!anonymous namespace\)).*$", "", d) for m, d in zip(names, out)}   # (no return type, no parameter list)


def kernels(path):
    """{mangled name: (instruction lines, descriptor lines, kernarg size)} of an assembly file"""
    text = open(path).read()
    found = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", text, re.M | re.S):
        name, desc = m.group(1), m.group(2)
        body = text[text.index("\n%s:" % name):m.start()]
        lines = []
        for ln in body.split("\n")[2:]:
            ln = re.sub(r"\s+", " ", ln.split(";")[0]).strip().replace(name, "KERNEL")
            ln = re.sub(r"\.L(BB|tmp|func_begin)\d+(_\d+)?", lambda g: ".L" + g.group(1) + (g.group(2) or ""), ln)
            if ln and not ln.startswith((".section", ".p2align")):
                lines.append(ln)
        karg = re.search(r"\.amdhsa_kernarg_size (\d+)", desc).group(1)
        desc = [re.sub(r"\s+", " ", ln).strip().replace(name, "KERNEL") for ln in desc.split("\n") if "kernarg_size" not in ln]
        found[name] = (lines, desc, int(karg))
    return found


def remarks(path):
    """{mangled name: {remark: value}}"""
    res, cur = {}, None
    for ln in open(path):
        m = re.search(r"remark:\s+(.*?): (.*?) \[-Rpass-analysis", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = res.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    return res


def compare(before, after):
    bad = 0
    sides = []
    for p in (before, after):
        k, r = kernels(p), remarks(os.path.splitext(p)[0] + ".remarks")
        d = demangle(sorted(k))
        sides.append({d[n]: k[n] + (r.get(n, {}),) for n in k})
    a, b = sides
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("  %s: only %s" % (name, "before" if name in a else "after"))
            bad += 1
            continue
        what = []
        if a[name][0] != b[name][0]:
            what.append("instructions differ (%d / %d lines)" % (len(a[name][0]), len(b[name][0])))
        if a[name][1] != b[name][1]:
            what.append("descriptor differs")
        if a[name][3] != b[name][3]:
            what.append("resources differ: " + ", ".join("%s %s -> %s" % (k, a[name][3].get(k), v) for k, v in b[name][3].items() if a[name][3].get(k) != v))
        if a[name][2] != b[name][2]:
            print("  %s: kernarg size %d -> %d" % (name, a[name][2], b[name][2]))
        if what:
            print("  %s: %s" % (name, "; ".join(what)))
            bad += 1
    print("%s: %d kernels compared, %d differ" % (os.path.basename(after), len(set(a) & set(b)), bad))
    return bad


if __name__ == "__main__":
    args = sys.argv[1:]
    sys.exit(1 if sum(compare(args[i], args[i + 1]) for i in range(0, len(args), 2)) else 0)
