#!/usr/bin/env bash
# A/B the bench across library builds / env settings, interleaved rounds, one process per run:
#   scripts/ab.sh lib1.so lib2.so[@VAR=VALUE] ...   (ROUNDS, BENCH_ARGS from the environment)
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
mkdir -p gpurun_out
ROUNDS=${ROUNDS:-2}
ERR=$(mktemp -t ab_last.XXXXXX.err)  # the last bench run's stderr
for r in $(seq 1 $ROUNDS); do
  for spec in "$@"; do
    lib=${spec%%@*}; envs=""; [ "$spec" != "$lib" ] && envs=${spec#*@}
    out=$(env SPT_LIB=$lib $envs timeout -k 10 120 python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline ${BENCH_ARGS:-} 2>"$ERR") || { echo "$spec FAILED (stderr: $ERR)"; exit 1; }
    echo "$spec $(echo "$out" | python -c 'import json,sys; d=json.loads(sys.stdin.read()); print(d["value"], d["roofline"]["kernel_ms"])')"
  done
done | tee gpurun_out/ab.txt
