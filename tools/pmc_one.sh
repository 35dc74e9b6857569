#!/bin/bash
# one rocprofv3 --pmc pass over the config 3 probe: tools/pmc_one.sh <tag> COUNTER...
set -Ee
trap 'echo "pmc_one.sh: stopped, status $? at line $LINENO: $BASH_COMMAND" >&2' ERR
tag=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
out=$root/tools/out/$tag; mkdir -p $out
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --pmc "$@" -d $out/p -o p -- python $root/tools/perf_probe.py 1024 2 > $out/log.txt 2>&1
db=$(find $out/p -name '*.db' -print -quit)
python $root/tools/rocpd_summary.py "$db" | grep -E "ssk::k_(fft4096|time_domain)" | grep -v "^ *[0-9]+ +[0-9.]+ +[0-9.]+ +[0-9.]+ +[0-9.]+" | cut -c1-120
rm -rf $out/p
