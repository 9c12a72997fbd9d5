# Collects the rocprofv3 evidence of a round (run on the GPU box):
#   per workload: --kernel-trace --stats of the bench command (no counters), then separate --pmc passes
#   (gpurun refuses --pmc combined with tracing domains), then the un-profiled bench line.  The profiled runs skip bench.py's
#   counting launch (--no-stats): every kernel of a sequence then runs the same number of times, and a mean per launch is one population.
#   Every step runs under its own time limit (PROFILE_STEP_SECONDS, default 300; eight steps a workload), and the first one that fails ends
#   the script: nothing more is started on that GPU.
# Usage: bash tools/profile_round.sh <tag> [workload ...]     -> gpurun_out/prof_<tag>/<workload>/
tag=${1:-r03}; shift
wls=${@:-1k4c 1ppe 1azp-dna gso-1ppe gso-1k4c 2uuy}
cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
limit=${PROFILE_STEP_SECONDS:-300}
for w in $wls; do
  out=gpurun_out/prof_$tag/$w; mkdir -p $out
  B="python3 bench.py --full --workload $w --steps 10 --warmup 3 --cpu-seconds 0 --no-stats"
  timeout -k 10 $limit rocprofv3 --kernel-trace --stats --output-format csv -d $out/trace -- $B > $out/bench_traced.json 2> $out/trace.log || { echo "$w: the traced run failed"; tail -5 $out/trace.log; exit 1; }
  P="python3 bench.py --full --workload $w --steps 3 --warmup 1 --cpu-seconds 0 --no-stats"
  i=0
  while read -r set; do
    i=$((i+1))
    timeout -k 10 $limit rocprofv3 --pmc $set --output-format csv -d $out/pmc$i -- $P > /dev/null 2> $out/pmc$i.log || { echo "$w: counter pass $i failed"; tail -5 $out/pmc$i.log; exit 1; }
  done <<'SETS'
FETCH_SIZE
WRITE_SIZE
TCC_HIT_sum TCC_MISS_sum TCC_EA0_RDREQ_sum TCC_EA0_WRREQ_sum
SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS
SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_SALU SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_VMEM_WR SQ_ACTIVE_INST_SCA
TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum TCP_TOTAL_ACCESSES_sum TCP_PENDING_STALL_CYCLES_sum
SETS
  timeout -k 10 $limit python3 bench.py --full --workload $w --steps 10 --warmup 3 > $out/bench.json 2> $out/bench.err || { echo "$w: the bench run failed"; tail -5 $out/bench.err; exit 1; }
  python3 tools/summarize_profile.py $out > $out/summary.txt
  cat $out/summary.txt
done
