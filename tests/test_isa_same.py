"""tools/isa_same.py on small synthetic assembly: its four verdicts, and the exit code of each without and with --allow-renamed
(RENAMED is the only verdict the flag lets pass).  CPU test: no compiler, no GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "isa_same.py")

BODY = """\
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	s_load_dwordx2 s[2:3], s[4:5], 0x8
	v_lshlrev_b32_e32 v1, 3, v0
	s_waitcnt lgkmcnt(0)
	global_load_dwordx2 v[2:3], v1, s[0:1]
	s_cmp_lg_u32 s6, 0
	s_cbranch_scc1 .LBB0_2
; %bb.1:
	v_pk_mul_f32 v[2:3], v[2:3], s[2:3] op_sel_hi:[1,0]
.LBB0_2:
	s_waitcnt vmcnt(0)
	global_store_dwordx2 v1, v[2:3], s[0:1] offset:16
	s_endpgm
"""


def asm(body, name="k_probe"):
    return (f"\t.text\n\t.globl\t{name}\n\t.type\t{name},@function\n{name}:\n{body}.Lfunc_end0:\n"
            f"\t.size\t{name}, .Lfunc_end0-{name}\n\t.section\t.rodata\n\t.amdhsa_kernel {name}\n\t\t.amdhsa_next_free_vgpr 4\n"
            "\t.end_amdhsa_kernel\n")


# the two scalar pairs swap roles: same instructions, other register numbers
SWAPPED = BODY.replace("s[0:1]", "s[X]").replace("s[2:3]", "s[0:1]").replace("s[X]", "s[2:3]")

CASES = {
    # name: (old, new, verdict, exit code, exit code with --allow-renamed)
    "same": (asm(BODY), asm(BODY.replace(".LBB0_2", ".LBB7_9").replace("; %bb.1:", "; another comment")), "SAME", 0, 0),
    "renamed": (asm(BODY), asm(SWAPPED), "RENAMED", 1, 0),
    "opcode": (asm(BODY), asm(BODY.replace("v_pk_mul_f32", "v_pk_add_f32")), "DIFF", 1, 1),
    "immediate": (asm(BODY), asm(BODY.replace("offset:16", "offset:24")), "DIFF", 1, 1),
    "width": (asm(BODY), asm(BODY.replace("v[2:3], v1, s[0:1]", "v[2:3], v1, s[0:3]")), "DIFF", 1, 1),      # one class, another width
    "missing": (asm(BODY), asm(BODY, name="k_other"), "MISSING", 1, 1),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_verdict_and_exit_codes(case, tmp_path):
    old, new, verdict, rc_plain, rc_allowed = CASES[case]
    (tmp_path / "old.s").write_text(old)
    (tmp_path / "new.s").write_text(new)
    for flags, rc in (([], rc_plain), (["--allow-renamed"], rc_allowed)):
        r = subprocess.run([sys.executable, TOOL, *flags, str(tmp_path / "old.s"), str(tmp_path / "new.s")], capture_output=True, text=True)
        lines = r.stdout.strip().split("\n")
        assert all(line.split()[-1] == verdict for line in lines[:-1]) and len(lines) >= 2, r.stdout + r.stderr
        assert r.returncode == rc, (flags, r.stdout, r.stderr)
        # the summary counts the verdicts
        n = len(lines) - 1
        for v in ("SAME", "RENAMED", "DIFF", "MISSING"):
            assert f"{n if v == verdict else 0} {v}" in lines[-1], lines[-1]

