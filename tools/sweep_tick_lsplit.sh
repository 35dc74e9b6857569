#!/bin/bash
# tick time by the chunk length of SPLIT calls (needs tools/bin/tune.so, a -DSS_TUNING build): tools/sweep_tick_lsplit.sh [L ...]
# The first sweep point that fails or times out ends the sweep.
set -Ee -o pipefail
trap 'echo "sweep_tick_lsplit.sh: stopped at L_split $L, status $? at line $LINENO" >&2' ERR
for L in ${@:-30 40 48 50 60}; do
  echo "== L_split $L"
  SS_TD_LSPLIT=$L SOUNDSCOPE_HIP_LIB=tools/bin/tune.so timeout -k 10 120 python tools/probe_tick_host.py | grep -E "tick wall|wait|separate"
done
