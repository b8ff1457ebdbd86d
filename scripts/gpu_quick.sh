#!/bin/bash
# Parity tests, then a short bench per workload given in $WORKLOADS (default: c2 c3).
# Stops at the first failing GPU step.
set -u
cd "$(dirname "$0")/.." || exit 1
mkdir -p bench_out
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread -p no:cacheprovider \
  ${PYTEST_ARGS:-} > bench_out/gpu_tests.log 2>&1
rc=$?
tail -15 bench_out/gpu_tests.log
[ $rc -eq 0 ] || exit $rc
for wl in ${WORKLOADS:-c2 c3}; do
  timeout -k 10 300 python bench.py --full --workload $wl --steps ${STEPS:-30} --warmup 3 ${BENCH_ARGS:-} \
    > bench_out/bench_$wl.json 2> bench_out/bench_$wl.err || { tail -20 bench_out/bench_$wl.err; exit 1; }
  cat bench_out/bench_$wl.json
done
