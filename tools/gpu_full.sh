#!/bin/bash
# Full GPU pass: -m gpu suite, smoke(), default bench line with every section (bench.py --full),
# each time-limited, chained.  Output under $OUT, default out/full.
set -o pipefail
export TMPDIR=/tmp
OUT=${OUT:-out/full}
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $OUT/t_gpu.log 2>&1 \
  || { echo TESTFAIL; tail -40 $OUT/t_gpu.log; exit 1; }
tail -3 $OUT/t_gpu.log
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke(); print('SMOKE OK')" > $OUT/smoke.log 2>&1 \
  || { echo SMOKEFAIL; tail -20 $OUT/smoke.log; exit 1; }
tail -1 $OUT/smoke.log
timeout -k 10 400 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err \
  || { echo BENCHFAIL; tail $OUT/bench.err; exit 1; }
cat $OUT/bench.json
