#!/bin/bash
# L2 counters of k_fft16k_run at config 5 (where does its 1.33x input over-fetch come from?): separate --pmc passes over tools/probe_cfg5.py
# The first pass that fails or times out ends the series.
set -Ee
trap 'echo "pmc_cfg5_l2.sh: stopped, status $? at line $LINENO: $BASH_COMMAND" >&2' ERR
root=$(cd "$(dirname "$0")/.." && pwd)
out=$root/tools/out/${1:-pmc_c5_l2}; mkdir -p $out
cd /tmp && export TMPDIR=/tmp
: > $out/summary.txt
for grp in "TCC_HIT_sum TCC_MISS_sum" "TCC_REQ_sum TCC_READ_sum" "TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_32B_sum" "TCP_TCC_READ_REQ_sum"; do
  echo "## rocprofv3 --pmc $grp -- python tools/probe_cfg5.py 64" >> $out/summary.txt
  timeout -k 10 300 rocprofv3 --pmc $grp -d $out/p -o p -- python $root/tools/probe_cfg5.py 64 > $out/log.txt 2>&1
  db=$(find $out/p -name '*.db' -print -quit)
  python $root/tools/rocpd_summary.py "$db" | grep "k_fft16k_run" | grep -v "^ *[0-9]+ +[0-9.]+ +[0-9.]+ +[0-9.]+ +[0-9.]+" | cut -c1-130 >> $out/summary.txt
  rm -rf $out/p
done
cat $out/summary.txt
