#!/bin/bash
# A/B of prebuilt library variants on ONE box WITHOUT touching the installed library: every run loads
# lightdock-rust_amd/lib/variants/<name>.so through LIGHTDOCK_HIP_VARIANT (lightdock-rust_amd/__init__.py).
# Usage (on the GPU box): bash tools/ab6.sh <rounds> [bench args...]      -- interleaves the variants <rounds> times, the order
# rotated by one from round to round (no library always runs first); every run under its own
# `timeout` (AB6_RUN_SECONDS, default 120: a caller with a time budget of its own sizes it so that rounds x variants x limit fits), and a
# run that fails ends the script.  "base" = the installed library.
set -u
shopt -s nullglob
cd "${GRAFT_REPO_ROOT:-/root/repo}" || exit 1
rounds=${1:-2}; shift
L=lightdock-rust_amd/lib
line() { python3 -c "import sys,json
try:
    d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('%.0f evals/s  step %.4f (min %.4f med %.4f) ms  kernel %.4f ms' % (d['value'], d['ms_per_step'], d.get('ms_per_step_min',0), d.get('ms_per_step_median',0), d['roofline']['kernel_ms']))
except Exception as e: print('FAILED', e)"; }
names=(base); for v in $L/variants/*.so; do names+=("$(basename "$v" .so)"); done
for round in $(seq 1 "$rounds"); do
  for k in $(seq 0 $((${#names[@]} - 1))); do
    n=${names[$(((k + round - 1) % ${#names[@]}))]}
    if [ "$n" = base ]; then v=""; else v=$n; fi
    out=$(LIGHTDOCK_HIP_VARIANT=$v timeout -k 10 "${AB6_RUN_SECONDS:-120}" python3 bench.py --full --cpu-seconds 0 "$@" 2>&1) || { echo "$n FAILED"; echo "$out" | tail -5; exit 1; }
    echo "$n $(echo "$out" | line)"
  done
done
