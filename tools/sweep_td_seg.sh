#!/bin/bash
# segment-length sweep of k_time_domain (sub-blocks per segment; needs a -DSS_TUNING build): tools/sweep_td_seg.sh <rate> <ch> <streams> seg...
# The first sweep point that fails or times out ends the sweep.
set -Ee -o pipefail
trap 'echo "sweep_td_seg.sh: stopped at seg=$s, status $? at line $LINENO" >&2' ERR
rate=$1; ch=$2; streams=$3; shift 3
lib=$(realpath tools/bin/tune.so)
for s in "$@"; do
  if [ "$s" = "auto" ]; then SOUNDSCOPE_HIP_LIB=$lib timeout -k 10 600 python tools/sweep_td_chunk.py $rate $ch $streams auto | sed "s/^/seg=auto /"
  else SS_TD_SEG_SUB=$s SOUNDSCOPE_HIP_LIB=$lib timeout -k 10 600 python tools/sweep_td_chunk.py $rate $ch $streams auto | sed "s/^/seg=$s /"; fi
done
