#!/usr/bin/env python3
"""The tile loop of ONE k_time_domain instantiation, block by block: the static side of the kernel's instruction budget.

    hipcc --offload-arch=gfx950 <the Makefile's CXXFLAGS> --cuda-device-only -S -o td_f4.s soundscope_amd/csrc/ss_td_f4.hip
    tools/isa_tile_budget.py td_f4.s "k_time_domain<4, false, 2, 2, 4, false, false>" [--trips pass1=6,pass2=6,...] [--json]

The instantiation is named as c++filt prints it (template arguments included, `ssk::` and the parameter list left out).  The tile
loop is found from the phase marks the kernel carries anyway: SS_PROF_MARK issues an s_setprio at every phase boundary, and the tile
loop is the innermost backward branch whose span holds every block with one.  Printed per basic block of that span: VALU, SALU,
LDS and VMEM instruction counts, the VALU count split into f64 arithmetic (of which v_mul_f64), packed f32 (v_pk_*), conversions
(v_cvt_*), lane moves (DPP operands, v_readlane / v_readfirstlane / v_writelane / v_permlane) and everything else, the phase (the
index of the last mark in front of the block, in layout order) and where the block branches.  A block that branches to itself is an
inner loop; the two inner loops with the most f64 arithmetic are the batch loops of the K-weighting passes (five samples a trip),
the one with more of it is pass 2 (`pass2`), the other pass 1 (`pass1`).

--trips weights blocks for one tile of a given shape (role or block index = trips; every other block of the span counts once):
the sum is printed as `weighted`.  Static counts need no weights; the sum over the span is `static`.
Nothing else of the assembly is looked at."""
import argparse
import json
import re
import subprocess
import sys

KINDS = ("valu", "f64", "mul_f64", "packed", "cvt", "move", "salu", "lds", "vmem", "wait")


def demangle(names):
    out = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    return [re.sub(r"^void ", "", n.split("(")[0]).replace("ssk::", "") for n in out]


def kernel_text(asm, want):
    """(mangled name, lines of the function body, {resource: value} from its .amdhsa / comment footer)"""
    names = re.findall(r"^(_Z\S+):\s*; @", asm, re.M)
    plain = demangle(names) if names else []
    hits = [m for m, p in zip(names, plain) if p == want]
    if not hits:
        raise SystemExit(f"no kernel named {want!r} among {len(names)} functions")
    name = hits[0]
    i = asm.index("\n" + name + ":")
    j = asm.index(".Lfunc_end", i)
    k = asm.find("\n\t.text", j)
    foot = asm[j:k if k > 0 else j + 20000]
    res = {}
    for key, pat in (("vgprs", r"; NumVgprs: (\d+)"), ("agprs", r"; NumAgprs: (\d+)"), ("sgprs", r"; NumSgprs: (\d+)"),
                     ("scratch", r"; ScratchSize: (\d+)"), ("occupancy", r"; Occupancy: (\d+)"), ("lds", r"; LDSByteSize: (\d+)")):
        m = re.search(pat, foot)
        if m:
            res[key] = int(m.group(1))
    return name, asm[i:j].split("\n")[2:], res


def classify(ins):
    op = ins.split()[0]
    if op.startswith(("s_waitcnt", "s_nop", "s_setprio", "s_sleep", "s_barrier")):
        return ["wait"]
    if op.startswith("s_"):
        return ["salu"]
    if op.startswith("ds_"):
        return ["lds"]
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return ["vmem"]
    if op.startswith("v_"):
        k = ["valu"]
        if "_f64" in op and op.startswith(("v_fma", "v_mul", "v_add", "v_fmac", "v_min", "v_max")):
            k.append("f64")
            if op.startswith("v_mul_f64"):
                k.append("mul_f64")
        elif op.startswith("v_pk_"):
            k.append("packed")
        elif op.startswith("v_cvt"):
            k.append("cvt")
        elif ("dpp" in ins or "row_" in ins or "quad_perm" in ins or "wave_sh" in ins
              or op.startswith(("v_readlane", "v_readfirstlane", "v_writelane", "v_permlane"))):
            k.append("move")
        return k
    return []


def blocks_of(lines):
    blocks = [{"label": "entry", "ins": []}]
    for l in lines:
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            blocks.append({"label": m.group(1), "ins": []})
            continue
        t = l.strip()
        if not t or t[0] in ";.":
            continue
        blocks[-1]["ins"].append(t.split(";")[0].strip())
    idx = {b["label"]: k for k, b in enumerate(blocks)}
    for k, b in enumerate(blocks):
        b["count"] = {q: 0 for q in KINDS}
        b["marks"], b["to"] = [], []
        for ins in b["ins"]:
            for q in classify(ins):
                b["count"][q] += 1
            if ins.startswith("s_setprio"):
                b["marks"].append(int(ins.split()[1]))
            m = re.match(r"s_cbranch_\w+ (\.LBB\d+_\d+)|s_branch (\.LBB\d+_\d+)", ins)
            if m:
                b["to"].append(idx.get(m.group(1) or m.group(2), -1))
    return blocks


def tile_loop(blocks):
    marked = [k for k, b in enumerate(blocks) if b["marks"]]
    if not marked:
        raise SystemExit("no s_setprio phase marks in this kernel")
    lo, hi = min(marked), max(marked)
    spans = [(t, k) for k, b in enumerate(blocks) for t in b["to"] if 0 <= t <= k and t <= lo and k >= hi]
    if not spans:
        raise SystemExit("no backward branch spans the phase marks")
    return min(spans, key=lambda s: s[1] - s[0])


def analyse(asm, want, trips):
    name, lines, res = kernel_text(asm, want)
    blocks = blocks_of(lines)
    first, last = tile_loop(blocks)
    # phase of a block: marks seen so far in layout order (the body is laid out in program order; the index counts marks, the
    # priority value alone is ambiguous: {0, 3, 2, 3, 1, 1, 0, 0})
    nmarks = 0
    rows = []
    for k in range(first, last + 1):
        b = blocks[k]
        rows.append({"block": k, "label": b["label"], "phase_marks_before": nmarks, "self_loop": k in b["to"],
                     "to": b["to"], "prio": b["marks"], **b["count"]})
        nmarks += len(b["marks"])
    inner = sorted((r for r in rows if r["self_loop"] and r["f64"] > 0), key=lambda r: -r["f64"])[:2]
    roles = {}
    if len(inner) == 2:
        roles["pass2"], roles["pass1"] = inner[0]["block"], inner[1]["block"]
    for r in rows:
        r["role"] = next((n for n, k in roles.items() if k == r["block"]), "")
    static = {q: sum(r[q] for r in rows) for q in KINDS}
    weighted = None
    if trips is not None:
        w = {}
        for key, n in trips.items():
            w[roles[key] if key in roles else int(key)] = n
        weighted = {q: sum(r[q] * w.get(r["block"], 1) for r in rows) for q in KINDS}
    return {"kernel": want, "mangled": name, "resources": res, "tile_loop": [first, last], "roles": roles, "blocks": rows,
            "static": static, "weighted": weighted, "trips": trips}


def render(a):
    out = [f"kernel {a['kernel']}",
           "resources " + " ".join(f"{k}={v}" for k, v in sorted(a["resources"].items())),
           f"tile loop: blocks {a['tile_loop'][0]} .. {a['tile_loop'][1]}" + "".join(f", {n} = block {k}" for n, k in sorted(a["roles"].items())),
           f"{'#':>4} {'label':<11} {'ph':>2} {'VALU':>5} {'f64':>4} {'mul64':>5} {'pk':>4} {'cvt':>4} {'move':>4} {'SALU':>5} {'LDS':>4} {'VMEM':>4}  notes"]
    for r in a["blocks"]:
        notes = [r["role"]] if r["role"] else []
        notes += [f"prio{p}" for p in r["prio"]]
        notes += [("^" if t <= r["block"] else "v") + str(t) for t in r["to"]]
        out.append(f"{r['block']:>4} {r['label']:<11} {r['phase_marks_before']:>2} {r['valu']:>5} {r['f64']:>4} {r['mul_f64']:>5} {r['packed']:>4} "
                   f"{r['cvt']:>4} {r['move']:>4} {r['salu']:>5} {r['lds']:>4} {r['vmem']:>4}  " + " ".join(notes))
    for tag in ("static", "weighted"):
        t = a[tag]
        if t is None:
            continue
        head = tag if tag == "static" else "weighted (" + ",".join(f"{k}={v}" for k, v in a["trips"].items()) + ")"
        out.append(f"{head}: VALU {t['valu']} (f64 {t['f64']} of which v_mul_f64 {t['mul_f64']}, packed {t['packed']}, cvt {t['cvt']}, "
                   f"lane moves {t['move']}), SALU {t['salu']}, LDS {t['lds']}, VMEM {t['vmem']}")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("kernel")
    ap.add_argument("--trips", default=None, help="role-or-block=trips,... (weights for one tile)")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    trips = None
    if args.trips:
        trips = {k: int(v) for k, v in (kv.split("=") for kv in args.trips.split(","))}
    a = analyse(open(args.asm).read(), args.kernel, trips)
    print(json.dumps(a) if args.json else render(a))


if __name__ == "__main__":
    sys.exit(main())
