#!/bin/bash
# Bench plus a rocprofv3 kernel + memory-copy trace of the same command (diagnosis of the timed loop).
set -u
cd "$(dirname "$0")/.." || exit 1
export TMPDIR=/tmp
mkdir -p bench_out/diag
timeout -k 10 300 python3 bench.py --full ${BENCH_ARGS:---steps 30 --warmup 3} > bench_out/diag/bench.json 2> bench_out/diag/bench.err || exit $?
cat bench_out/diag/bench.json >&2
timeout -k 10 300 rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d bench_out/diag/prof -o run -- \
  python3 bench.py --full --steps 30 --warmup 3 --no-cpu-baseline ${BENCH_ARGS:-} > bench_out/diag/prof_bench.json 2> bench_out/diag/prof_bench.err
