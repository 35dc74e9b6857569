#!/bin/bash
# windows per spectrum workgroup sweep on the config 3 probe (needs a -DSS_TUNING build: tools/bin/tune.so)
# The first sweep point that fails or times out ends the sweep.
set -Ee -o pipefail
trap 'echo "sweep_wpb.sh: stopped at SS_FFT_WPB=$w, status $? at line $LINENO" >&2' ERR
for w in "$@"; do
  echo "=== SS_FFT_WPB=$w"
  SS_FFT_WPB=$w SOUNDSCOPE_HIP_LIB=$(realpath tools/bin/tune.so) timeout -k 10 600 python tools/perf_probe.py 1024 8 | grep -E "fft4096"
done
