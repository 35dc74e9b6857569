#!/usr/bin/env python3
"""The window loop of ONE kernel of an AMDGPU assembly file as counts and as a sequence — the static side of the spectrum kernels'
instruction budget, beside tools/isa_blocks.py, which gives the same kernel block by block:

    tools/isa_loop.py <file.s> <mangled-name substring>           the counts of the loop, one line
    tools/isa_loop.py <file.s> <mangled-name substring> --seq     its v_pk_* / v_log_f32 instructions in program order, registers
                                                                  replaced by their width (v2 = a pair), one per line: two builds
                                                                  that differ only in scheduling elsewhere give the same text

The loop is the outermost loop (the compiler's `Loop Header: Depth=1` / `in Loop: Header=` block comments) that holds the most
packed instructions: the window loop of k_fft4096_ms1.  Every block of it is counted once, the rare ones (exact-energy exponent,
rescale, zero bins, floor rows) included.  Counts: packed (v_pk_*), valu (every other v_* instruction, moves and DPP included),
div (v_div_* and v_rcp_f32), log (v_log_f32)."""
import re
import sys


def kernel_text(s, sub):
    names = [m for m in re.findall(r'^(\S+):\s*; @', s, re.M) if sub in m]
    assert names, "no kernel matches " + sub
    i = s.index('\n' + names[0] + ':')
    return names[0], s[i:s.index('.Lfunc_end', i)]


def loops(text):
    """{header label: [instruction lines]} of the depth-1 loops, in program order"""
    out, cur = {}, None
    for l in text.split('\n'):
        if re.match(r'^(\.LBB\d+_\d+:|; %bb\.\d+:)', l):
            m = re.search(r'in Loop: Header=(BB\d+_\d+) Depth=(\d+)', l)
            if m:
                # a block of an inner loop names its own header: walk up is not needed, the kernels' hot loops hold no inner loop
                cur = m.group(1) if m.group(2) == '1' else cur
            elif 'Loop Header: Depth=1' in l:
                cur = re.match(r'^\.L(BB\d+_\d+):', l).group(1)
            elif 'Loop' not in l:
                cur = None
            continue
        t = l.strip()
        if cur is None or not t or t[0] in ';.':
            continue
        out.setdefault(cur, []).append(t)
    return out


def shape(ins):
    """an instruction with its registers replaced by their width"""
    def reg(m):
        return "%s<%d>" % (m.group(1), int(m.group(3)) - int(m.group(2)) + 1 if m.group(2) else 1)
    return re.sub(r'\b([vs])(?:\[(\d+):(\d+)\]|\d+\b)', reg, ins)


def analyse(s, sub):
    name, text = kernel_text(s, sub)
    lp = loops(text)
    head = max(lp, key=lambda h: sum(i.startswith('v_pk_') for i in lp[h]))
    ins = lp[head]
    ops = [i.split()[0] for i in ins]
    return {"kernel": name, "header": head,
            "packed": sum(o.startswith('v_pk_') for o in ops),
            "valu": sum(o.startswith('v_') and not o.startswith('v_pk_') for o in ops),
            "div": sum(o.startswith('v_div_') or o.startswith('v_rcp_f32') for o in ops),
            "log": sum(o.startswith('v_log_f32') for o in ops),
            "seq": [shape(i) for i in ins if i.startswith(('v_pk_', 'v_log_f32'))]}


if __name__ == "__main__":
    r = analyse(open(sys.argv[1]).read(), sys.argv[2])
    if "--seq" in sys.argv:
        print("\n".join(r["seq"]))
    else:
        print("%s: window loop %s: packed %d, other VALU %d, v_div_* / v_rcp_f32 %d, v_log_f32 %d"
              % (r["kernel"], r["header"], r["packed"], r["valu"], r["div"], r["log"]))
