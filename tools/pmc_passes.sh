#!/bin/bash
# PMC passes (one rocprofv3 run per counter group; no tracing) over tools/perf_probe.py.
# usage: [PROBE=tools/probe_native.py] tools/pmc_passes.sh <tag> "<probe args>" "<group1 counters>" "<group2 counters>" ...
# The first pass that fails or times out ends the series.
set -Eeu
trap 'echo "pmc_passes.sh: stopped at group ${i:-0}, status $? at line $LINENO: $BASH_COMMAND" >&2' ERR
tag=$1; shift
args=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
out=$root/tools/out/$tag
mkdir -p "$out"
cd /tmp && export TMPDIR=/tmp
i=0
for grp in "$@"; do
  i=$((i+1))
  timeout -k 10 300 rocprofv3 --pmc $grp -d $out/g$i -o p -- python $root/${PROBE:-tools/perf_probe.py} $args > $out/g$i.log 2>&1
  db=$(find $out/g$i -name '*.db' -print -quit)
  echo "## group $i: $grp" >> $out/summary.txt
  python $root/tools/rocpd_summary.py "$db" | grep -E "ssk::" | grep -v "^ *[0-9]+ +[0-9.]+ +[0-9.]+ +[0-9.]+ +[0-9.]+ +[0-9.]+ +None" >> $out/summary.txt
  rm -rf $out/g$i
done
cat $out/summary.txt
