#!/bin/bash
# Which hardware queue does a session's loudness chain run on, and what does a tick look like on a slow one?
# (rocprofv3 kernel trace over tools/probe_tick_sessions.py, timelines by tools/tick_timeline.py)
set -Eeu
trap 'echo "probe_tick_queues.sh: stopped, status $? at line $LINENO: $BASH_COMMAND" >&2' ERR
root=$(cd "$(dirname "$0")/.." && pwd)
out=$root/tools/out/${1:-tick_queues}
mkdir -p "$out"
cd /tmp && export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace -d $out/kt -o kt -- python $root/tools/probe_tick_sessions.py > $out/sessions.log 2>&1
db=$(find $out/kt -name '*.db' -print -quit)
[ -n "$db" ] && python $root/tools/tick_timeline.py "$db" 1 > $out/timeline.txt
rm -rf $out/kt
grep -v rocprofv3 $out/sessions.log; cat $out/timeline.txt
