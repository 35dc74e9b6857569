"""The development builds still compile.  CPU test: every product translation unit of the Makefile is checked by hipcc -fsyntax-only (host and
gfx950 device front ends) under each kept build configuration, with the Makefile's own flags and source list.

Those configurations are the only compile-time variants of the library besides the release build: -DSS_TUNING (environment knobs of the
sweep and probe tools), -DSS_TD_PROF / -DSS_FFT_PROF (shader-clock phase profiles, ss_debug_td_prof / ss_debug_fft_prof) and
-DSS_TD_TRACE (the tile trace, ss_debug_td_trace; built together with SS_TUNING)."""
import os
import re
import shlex
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "soundscope_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
CONFIGS = [["-DSS_TUNING"], ["-DSS_TD_PROF"], ["-DSS_FFT_PROF"], ["-DSS_TUNING", "-DSS_TD_TRACE"]]


def _makefile_var(name):
    with open(os.path.join(CSRC, "Makefile")) as f:
        m = re.search(rf"^{name}\s*[:?]?=\s*(.*)$", f.read(), re.M)
    assert m, f"{name} not found in the Makefile"
    return shlex.split(m.group(1))


def _check(job):
    defines, src = job
    lang = ["-x", "hip"] if src.endswith(".cpp") else []
    cmd = [HIPCC, "--offload-arch=gfx950", *_makefile_var("CXXFLAGS"), *defines, *lang, "-fsyntax-only", src]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    return (" ".join(defines) + " " + src, r.returncode, r.stderr[-2000:])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc in this environment")
def test_kept_development_builds_compile():
    srcs = _makefile_var("SRCS")
    assert len(srcs) >= 15 and all(os.path.exists(os.path.join(CSRC, s)) for s in srcs)
    jobs = [(d, s) for d in CONFIGS for s in srcs]
    with ThreadPoolExecutor(max(1, min(8, os.cpu_count() or 1))) as ex:
        results = list(ex.map(_check, jobs))
    bad = [f"{name}:\n{err}" for name, rc, err in results if rc != 0]
    assert not bad, "development builds that do not compile:\n" + "\n".join(bad)
