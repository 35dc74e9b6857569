#!/bin/bash
# kernel durations and HIP API totals of the Analyzer path's get_fft (300 calls, warm)
set -Ee
trap 'echo "probe_getfft_trace.sh: stopped, status $? at line $LINENO: $BASH_COMMAND" >&2' ERR
root=$(cd "$(dirname "$0")/.." && pwd)
out=$root/tools/out/r6e; mkdir -p $out
cd /tmp && export TMPDIR=/tmp
cat > /tmp/gf.py <<PY
import sys, time
sys.path.insert(0, "$root"); sys.path.insert(0, "$root/tests")
import numpy as np
import soundscope_amd as ssa
from conftest import make_stereo
x = make_stereo(1, 48000 * 4, 48000)
mid, side = ssa.get_mid_and_side_samples(x)
an = ssa.Analyzer(); an.create_loudness_meter(2, 48000)
for k in range(300): an.get_fft(mid[k * 100:k * 100 + 16384])
t0 = time.perf_counter()
for k in range(300): an.get_fft(mid[k * 100:k * 100 + 16384])
print("get_fft wall", (time.perf_counter() - t0) / 300 * 1e6, "us")
PY
timeout -k 10 600 rocprofv3 --hip-trace --kernel-trace --stats -f csv -d $out/ht -o ht -- python /tmp/gf.py > $out/run.log 2>&1
grep "get_fft wall" $out/run.log
f=$(find $out/ht -name '*hip_api_stats.csv' -print -quit); head -8 "$f" | cut -d, -f1-7
f=$(find $out/ht -name '*kernel_stats.csv' -print -quit); head -4 "$f" | cut -d, -f1-7
rm -rf $out/ht
timeout -k 10 300 python /tmp/gf.py
