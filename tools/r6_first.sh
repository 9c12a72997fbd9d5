#!/bin/bash
# round 6, first GPU call: the parity suite on the round's first edits, the two microbenchmarks, a baseline of the headline
cd "${GRAFT_REPO_ROOT:?}" || exit 1
out=${1:?usage: bash tools/r6_first.sh <output directory>}; mkdir -p "$out"
( cd tools/microbench && timeout 300 ./mfma_batch 2000 ) > $out/mfma_batch.txt 2>&1
( cd tools/microbench && timeout 300 ./valu_rate ) > $out/valu_rate.txt 2>&1
timeout 1500 python -m pytest tests -m gpu -x -q > $out/pytest.txt 2>&1
for i in 1 2 3; do timeout 200 python bench.py --full --cpu-seconds 0 > $out/bench_$i.json 2> $out/bench_$i.err; done
timeout 300 python bench.py --full > $out/bench_full.json 2> $out/bench_full.err
timeout 200 python bench.py --full --workload 2uuy --cpu-seconds 0 > $out/bench_2uuy.json 2>&1
tail -3 $out/pytest.txt; cat $out/mfma_batch.txt; tail -16 $out/valu_rate.txt
python - "$out" <<'PY'
import json,glob,sys
for f in sorted(glob.glob(sys.argv[1] + '/bench_*.json')):
    try:
        d=json.loads(open(f).read().strip().splitlines()[-1]); print(f, '%.0f'%d['value'], d['ms_per_step'], d.get('ms_per_step_min'), d.get('ms_per_step_median'), d.get('ms_per_step_max'), d['roofline']['kernel_ms'])
    except Exception as e: print(f, 'FAILED', e)
PY
