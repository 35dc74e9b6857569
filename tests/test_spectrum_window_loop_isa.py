"""The window loop of the two k_fft4096_ms1 instantiations holds no launch constant and no dead move: tools/isa_loop.py on the
cross-compiled kernels (hipcc for gfx950 with the Makefile's flags, device only, no GPU needed) must find
  * no v_div_* and no v_rcp_f32 in any block of the loop (the log operand of a zero magnitude is FftBatchParams::lg0, formed on
    the host),
  * as many packed instructions as the parent of that change had (the transform and the squared magnitudes are untouched),
  * at least 40 fewer other VALU instructions than the parent had,
the parent's figures being the `== parent` lines of profiles/spectrum_window_loop_isa.txt (written with the same tool at that
commit).  Every block of the loop counts once, the rare ones included."""
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
LEDGER = os.path.join(ROOT, "profiles", "spectrum_window_loop_isa.txt")
KERNELS = {"k_fft4096_ms1<4, 12, false>": "k_fft4096_ms1ILi4ELi12ELb0E", "k_fft4096_ms1<4, 12, true>": "k_fft4096_ms1ILi4ELi12ELb1E"}


def _tool():
    spec = importlib.util.spec_from_file_location("isa_loop", os.path.join(ROOT, "tools", "isa_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def loops(tmp_path_factory):
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.skip("no hipcc / c++filt in this environment")
    asm = str(tmp_path_factory.mktemp("isa") / "ss_fft.s")
    r = subprocess.run([HIPCC, *FLAGS, "--cuda-device-only", "-S", "-o", asm, "ss_fft.hip"], cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(asm) as f:
        text = f.read()
    tool = _tool()
    return {name: tool.analyse(text, mangled) for name, mangled in KERNELS.items()}


def _parent(name):
    with open(LEDGER) as f:
        text = f.read()
    m = re.search(r"^== parent +" + re.escape(name) + r": window loop \S+: packed (\d+), other VALU (\d+)", text, re.M)
    assert m, "profiles/spectrum_window_loop_isa.txt carries no parent line for " + name
    return int(m.group(1)), int(m.group(2))


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_no_division_in_the_window_loop(loops, name):
    assert loops[name]["div"] == 0, loops[name]["div"]
    assert loops[name]["log"] >= 16, loops[name]["log"]          # (the right loop: sixteen dB values per lane and window)


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_packed_count_is_the_parents(loops, name):
    assert loops[name]["packed"] == _parent(name)[0], (loops[name]["packed"], _parent(name))


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_forty_fewer_other_valu_than_the_parent(loops, name):
    assert loops[name]["valu"] <= _parent(name)[1] - 40, (loops[name]["valu"], _parent(name))
