# GPU box: the default bench.py line of every workload with the committed profiles/traffic.json in place
# (-> <output directory>/r04_<workload>_bench.json; copied to profiles/ by hand)   usage: bash tools/r4_bench_all.sh <output directory>
cd $GRAFT_REPO_ROOT
out=${1:?usage: bash tools/r4_bench_all.sh <output directory>}; mkdir -p "$out"
for w in 1k4c 1ppe 1azp-dna gso-1ppe gso-1k4c 2uuy; do
  n=$(echo $w | tr - _)
  if [ $w = 1k4c ]; then timeout 600 python bench.py --full > "$out/r04_${n}_bench.json" 2> "$out/r04_${n}_bench.err"
  else timeout 600 python bench.py --full --workload $w > "$out/r04_${n}_bench.json" 2> "$out/r04_${n}_bench.err"; fi
  tail -1 "$out/r04_${n}_bench.json" | cut -c1-120
done
