"""The static instruction budget of the flagship time-domain instantiation is gated with the code: tools/isa_tile_budget.py on the
cross-compiled `k_time_domain<4, false, 2, 2, 4, false, false>` (hipcc for gfx950 with the Makefile's flags, device only, no GPU
needed) must find no scratch, at most 128 VGPRs, no `v_mul_f64` in the batch loop of the second K-weighting pass (the unit-gain
output taps: four FMAs per sample), and fewer VALU instructions in one tile's walk through the loop than the parent of that change
had — the `weighted` figure recorded in profiles/td_tile_ledger.txt: the batch loops of the two passes six times (a 30-frame chunk is
six batches of five), every other block once.  (The plain sum over the blocks is not the measure: the loop also holds the
step-by-step form with gained taps that only a tile with a non-finite value in reach runs.)"""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "soundscope_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-slp-vectorize"]       # the Makefile's CXXFLAGS
KERNEL = "k_time_domain<4, false, 2, 2, 4, false, false>"
LEDGER = os.path.join(ROOT, "profiles", "td_tile_ledger.txt")


def _tool():
    spec = importlib.util.spec_from_file_location("isa_tile_budget", os.path.join(ROOT, "tools", "isa_tile_budget.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def ledger(tmp_path_factory):
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.skip("no hipcc / c++filt in this environment")
    asm = str(tmp_path_factory.mktemp("isa") / "ss_td_f4.s")
    r = subprocess.run([HIPCC, *FLAGS, "--cuda-device-only", "-S", "-o", asm, "ss_td_f4.hip"], cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(asm) as f:
        return _tool().analyse(f.read(), KERNEL, {"pass1": 6, "pass2": 6})


def _parent_valu():
    with open(LEDGER) as f:
        text = f.read()
    m = re.search(r"^== parent.*?^weighted \(pass1=6,pass2=6\): VALU (\d+)", text, re.M | re.S)
    assert m, "profiles/td_tile_ledger.txt carries no parent ledger"
    return int(m.group(1))


def test_flagship_build_fits_four_waves(ledger):
    res = ledger["resources"]
    assert res["scratch"] == 0, res
    assert res["vgprs"] <= 128 and res["occupancy"] == 4, res


def test_second_pass_has_no_f64_multiply(ledger):
    assert "pass2" in ledger["roles"] and "pass1" in ledger["roles"], ledger["roles"]
    rows = {r["block"]: r for r in ledger["blocks"]}
    p1, p2 = rows[ledger["roles"]["pass1"]], rows[ledger["roles"]["pass2"]]
    assert p2["mul_f64"] == 0, p2                           # unit-gain output taps: FMAs only
    assert p2["f64"] > p1["f64"] > 0, (p1, p2)              # (the roles are the right way round: pass 2 adds the taps and e += y^2)


def test_tile_loop_is_under_the_parents_valu_count(ledger):
    parent = _parent_valu()
    assert ledger["weighted"]["valu"] < parent, (ledger["weighted"]["valu"], parent)
