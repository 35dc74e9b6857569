#!/bin/bash
# k_time_domain's instruction counters by class, for one or more library builds (config 3 probe; one counter group per rocprofv3 run)
#   tools/pmc_td6.sh <tag> <lib|default> ...
# The first pass that fails or times out ends the series.
set -Eeu
trap 'echo "pmc_td6.sh: stopped at ${lib:--} group ${n:-0}, status $? at line $LINENO: $BASH_COMMAND" >&2' ERR
tag=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
out=$root/tools/out/$tag; mkdir -p $out
cd /tmp && export TMPDIR=/tmp
[ -f $out/counters_avail.txt ] || timeout -k 10 120 rocprofv3 -L > $out/counters_avail.txt 2>&1
for lib in "$@"; do
  echo "#### $lib" >> $out/summary.txt
  if [ "$lib" = default ]; then unset SOUNDSCOPE_HIP_LIB; else export SOUNDSCOPE_HIP_LIB=$(realpath $root/$lib); fi
  n=0
  for grp in "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VALU_FMA_F64" "SQ_INSTS_VALU_ADD_F64 SQ_INSTS_VALU_MUL_F64 SQ_INSTS_VALU_CVT SQ_INSTS_VALU_INT32" \
             "SQ_INSTS_VALU_ADD_F32 SQ_INSTS_VALU_FMA_F32 SQ_INSTS_VALU_MUL_F32 SQ_INSTS_MFMA" "SQ_INSTS_VALU_MFMA_F32 SQ_INSTS_VALU_MFMA_MOPS_F32 SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES" \
             "SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAVE_CYCLES SQ_WAIT_INST_ANY" "SQ_INST_CYCLES_VMEM SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS" \
             "SQ_INSTS_VALU_TRANS_F32 SQ_INSTS_VALU_INT64 SQ_INSTS_FLAT SQ_INSTS_SMEM"; do
    n=$((n + 1))
    echo "## --pmc $grp" >> $out/summary.txt
    timeout -k 10 300 rocprofv3 --pmc $grp -d $out/p$n -o p -- python $root/tools/perf_probe.py 1024 2 > $out/log_$n.txt 2>&1
    db=$(find $out/p$n -name '*.db' -print -quit)
    python $root/tools/rocpd_summary.py "$db" | grep -E "ssk::k_time_domain" | grep -v "^ *[0-9]+ +[0-9.]+ +[0-9.]+ +[0-9.]+ +[0-9.]+" | cut -c1-150 >> $out/summary.txt
    rm -rf $out/p$n
  done
done
cat $out/summary.txt
