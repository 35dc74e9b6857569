#!/usr/bin/env python3
"""Are the kernels of two AMDGPU assembly files the same machine code?  tools/isa_same.py [--allow-renamed] <old.s> <new.s>

The check of a refactor that must not move an instruction.  Make both files from one translation unit with the Makefile's flags
plus `--offload-device-only -S` (device-only compile, no GPU needed), e.g. in soundscope_amd/csrc:
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-slp-vectorize --offload-device-only -S -o new.s ss_fft.hip
A kernel is the text between its symbol label and the next `.Lfunc_end`; comments and assembler directives are dropped and the
basic-block labels are renumbered in order of appearance, so that only instructions and operands are compared.
Prints one line per kernel (name, instructions old, new, verdict) and a summary line that counts the verdicts:
  SAME     the two instruction lists are equal;
  RENAMED  they are equal once every register operand (vN, sN, aN, v[a:b], s[a:b], a[a:b]) is replaced by its class and width:
           the same instructions in the same order, the register allocator chose other numbers;
  DIFF     anything else;
  MISSING  a kernel only one file has, or whose body cannot be found.
Exits non-zero unless every kernel is SAME — or, with --allow-renamed, SAME or RENAMED."""
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


REG = re.compile(r"\b([vsa])(?:(\d+)|\[(\d+):(\d+)\])(?![\w\[])")


def classes(ins):
    """the instruction list with every register operand replaced by its class and width: v[4:5] -> v:2, s7 -> s:1"""
    return [REG.sub(lambda m: "%s:%d" % (m.group(1), 1 if m.group(2) else int(m.group(4)) - int(m.group(3)) + 1), i) for i in ins]


def verdict(old, new):
    if old is None or new is None:
        return "MISSING"
    if old == new:
        return "SAME"
    return "RENAMED" if classes(old) == classes(new) else "DIFF"


def count(ks, name):
    return sum(1 for i in ks[name] if not i.endswith(":")) if ks.get(name) is not None else "-"


def main():
    args = [a for a in sys.argv[1:] if a != "--allow-renamed"]
    if len(args) != 2:
        sys.exit(__doc__)
    passing = ("SAME", "RENAMED") if len(args) < len(sys.argv) - 1 else ("SAME",)
    old, new = kernels(args[0]), kernels(args[1])
    tally = dict.fromkeys(("SAME", "RENAMED", "DIFF", "MISSING"), 0)
    for name in sorted(set(old) | set(new)):
        v = verdict(old.get(name), new.get(name))
        tally[v] += 1
        print(f"{name}  {count(old, name)}  {count(new, name)}  {v}")
    print(f"{len(set(old) | set(new))} kernels: " + ", ".join(f"{n} {v}" for v, n in tally.items()))
    sys.exit(0 if all(tally[v] == 0 for v in tally if v not in passing) else 1)


if __name__ == "__main__":
    main()
