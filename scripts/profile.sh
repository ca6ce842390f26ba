#!/bin/bash
# Collects the rocprofv3 evidence for bench.py's roofline block (run on the GPU box).
#   1. kernel trace + stats           -> gpurun_out/prof/trace
#   2. PMC pass: FETCH_SIZE           -> gpurun_out/prof/pmc_fetch   (own run, no trace domains)
#   3. PMC pass: WRITE_SIZE           -> gpurun_out/prof/pmc_write
#   4. PMC pass: wave-level SQ counters (issue / wait / busy)  -> pmc_sq, beside the others
#   5. PMC pass: instruction mix (counters only, a run of its own)  -> pmc_mix, likewise
#      (five SQ counters of the eight slots; MIX_COUNTERS overrides the list where `rocprofv3 --list-avail` names the fp64
#      matrix count differently)
# Every pass runs under a time limit of its own and the script stops at the first one that fails.
# Summaries are copied into profiles/ by hand afterwards (profiles/ is tracked, gpurun_out/ is scratch).
set -u
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$ROOT/gpurun_out/prof
ARGS=${BENCH_ARGS:---steps 10 --warmup 2 --repeats 1 --no-cpu-baseline --no-latency --no-second-workload --no-copy-bandwidth}
MIX_COUNTERS=${MIX_COUNTERS:-SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VALU_MFMA_MOPS_F64 SQ_VALU_MFMA_BUSY_CYCLES}
PASS_LIMIT=${PASS_LIMIT:-300}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
pass() {  # log name, rocprofv3 arguments ...
  local log=$OUT/$1
  shift
  timeout -k 10 $PASS_LIMIT rocprofv3 "$@" -- python $ROOT/bench.py $ARGS > $log 2>&1
  local rc=$?
  if [ $rc -ne 0 ]; then
    echo "pass failed (exit status $rc): $log"
    tail -5 $log
    exit $rc
  fi
}
pass bench_trace.log --kernel-trace --stats -d $OUT/trace -o bench
pass bench_fetch.log --pmc FETCH_SIZE -d $OUT/pmc_fetch -o bench
pass bench_write.log --pmc WRITE_SIZE -d $OUT/pmc_write -o bench
pass bench_sq.log --pmc SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS -d $OUT/pmc_sq -o bench
pass bench_mix.log --pmc $MIX_COUNTERS -d $OUT/pmc_mix -o bench
cd $ROOT
timeout -k 10 $PASS_LIMIT python bench.py ${ARGS/--repeats 1/--repeats 5} > $OUT/bench_plain.log 2>&1 || { echo "plain run failed"; tail -5 $OUT/bench_plain.log; exit 1; }
find $OUT -type f | head -50
tail -2 $OUT/bench_plain.log
