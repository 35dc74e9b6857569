#!/bin/bash
# A/B of library builds on BASELINE config 5 (tools/probe_cfg5.py): tools/ab_cfg5.sh lib1.so lib2.so ...  ("default" = in-tree)
# The first build whose probe fails or times out ends the series.
set -Ee
trap 'echo "ab_cfg5.sh: stopped, status $? at line $LINENO: $BASH_COMMAND" >&2' ERR
for lib in "$@"; do
  echo "=== $lib"
  if [ "$lib" = "default" ]; then timeout -k 10 600 python tools/probe_cfg5.py 64
  else SOUNDSCOPE_HIP_LIB=$(realpath "$lib") timeout -k 10 600 python tools/probe_cfg5.py 64; fi
done
