#!/bin/bash
# All BASELINE.json configs on one GPU (c5 = the metric's workload), each with every
# section of the line (bench.py --full).  Output under $OUT, default out/bench_<tag>.
set -u
TAG=${1:-r01}
OUT=${OUT:-out/bench_$TAG}
mkdir -p $OUT
for c in ${CONFIGS:-c5 c2 c3 c4 c1}; do
  timeout -k 10 500 python3 bench.py --full --config $c ${EXTRA_ARGS:-} > $OUT/$c.json 2> $OUT/$c.err
  rc=$?
  echo "$c rc=$rc"; tail -c 600 $OUT/$c.json
  if [ $rc -ne 0 ]; then tail -5 $OUT/$c.err; fi
  if [ $rc -ge 124 ]; then exit $rc; fi
done
