#!/usr/bin/env python3
"""Are the kernels of two AMDGPU assembly files the same machine code?  tools/isa_same.py <old.s> <new.s>

The check of a refactor that must not move an instruction.  Make both files from one translation unit with the Makefile's flags
plus `--offload-device-only -S` (device-only compile, no GPU needed), e.g. in soundscope_amd/csrc:
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-slp-vectorize --offload-device-only -S -o new.s ss_fft.hip
A kernel is the text between its symbol label and the next `.Lfunc_end`; comments and assembler directives are dropped and the
basic-block labels are renumbered in order of appearance, so that only instructions and operands are compared.
Prints one line per kernel (name, instructions old, new, SAME / DIFF; MISSING for a kernel only one file has or whose body
cannot be found) and exits non-zero unless every kernel is SAME."""
import re
import sys


def kernels(path):
    """{symbol: [instruction, ...]} for every .amdhsa_kernel of the file; None where the kernel's label or end is not found"""
    s = open(path).read()
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", s, re.M):
        m = re.search(r"^" + re.escape(name) + r":", s, re.M)
        end = s.find(".Lfunc_end", m.end()) if m else -1
        if end < 0:
            out[name] = None
            continue
        body = s[m.end():end]
        ins, labels = [], {}
        for line in body.split("\n"):
            t = line.split(";", 1)[0].strip()
            if not t:
                continue
            lab = re.match(r"^(\.L\w+):$", t)
            if lab:
                labels.setdefault(lab.group(1), "L%d" % len(labels))
                ins.append(lab.group(1) + ":")
                continue
            if t[0] == ".":
                continue
            ins.append(re.sub(r"\s+", " ", t))
        pat = re.compile(r"\.L\w+")
        out[name] = [pat.sub(lambda q: labels.get(q.group(0), q.group(0)), i) for i in ins]
    return out


def count(ks, name):
    return sum(1 for i in ks[name] if not i.endswith(":")) if ks.get(name) is not None else "-"


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in sorted(set(old) | set(new)):
        if old.get(name) is None or new.get(name) is None:
            verdict = "MISSING"
        else:
            verdict = "SAME" if old[name] == new[name] else "DIFF"
        bad += verdict != "SAME"
        print(f"{name}  {count(old, name)}  {count(new, name)}  {verdict}")
    print(f"{len(set(old) | set(new))} kernels, {bad} not the same")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
