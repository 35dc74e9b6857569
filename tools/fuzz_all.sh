#!/bin/bash
# every randomised programme set, new seeds:  tools/fuzz_all.sh [first seed]      (logs under tools/out/fuzz_<seed>/; a summary line per set)
# The first set that fails or times out ends the campaign: the sets behind it are not started.
first=${1:-100000}
out=tools/out/fuzz_$first; mkdir -p $out
run() {
  local name=$1 rc=0; shift
  timeout -k 10 900 "$@" > $out/$name.log 2>&1 || rc=$?
  echo "$name rc $rc : $(grep -v '^GPU\|^Failed\|coredump' $out/$name.log | tail -1 | cut -c1-160)"
  grep "^FAIL" $out/$name.log | cut -c1-500 | head -5
  if [ $rc != 0 ]; then echo "fuzz_all.sh: stopped at $name (status $rc)" >&2; exit $rc; fi
}
for c in 0 1 2 3 4 5 6 7; do run batch_reuse_$c python tools/fuzz_batch.py 100 $((first + 100 * c)) --reuse; done
for c in 0 1; do run batch_big_$c python tools/fuzz_batch.py 100 $((first + 1000 + 100 * c)) --big; done
for c in 0 1; do run batch_wide_$c python tools/fuzz_batch.py 100 $((first + 2000 + 100 * c)) --wide; done
for c in 0 1 2 3 4 5; do run handle_$c python tools/fuzz_handle.py 100 $((first + 100 * c)); done
run columns python tools/fuzz_columns.py 500 $first
run render python tools/fuzz_render.py 300 $first
run pcm python tools/fuzz_pcm.py 500 $first
run ticks python tools/fuzz_ticks.py 1000 $first
run capture python tools/fuzz_capture.py 500 $first
run streaming python tools/fuzz_streaming.py 600 $first
