#!/bin/bash
# A/B two in-tree builds on the GPU box: libhpe.so (B) vs $1 (A, default libhpe_base.so).
# Usage (on the box): bash tools/ab.sh [libA.so] [rounds] [extra bench args]
# Logs go to $AB_OUT (default bench_out/ab); tools/ab_show.py summarises them.
set -o pipefail
A=${1:-libhpe_base.so}
R=${2:-2}
EXTRA=${3:-}
O=${AB_OUT:-bench_out/ab}
rm -rf $O; mkdir -p $O
for r in $(seq 1 $R); do
  for v in "$A" libhpe.so; do
    tag=$(basename $v .so)_$r
    HPE_LIB_VARIANT=$v timeout -k 10 200 python bench.py --full --steps 40 --no-cpu-baseline > $O/bench_$tag.log 2>&1 || exit 1
    if [ -n "$EXTRA" ]; then
      HPE_LIB_VARIANT=$v timeout -k 10 200 python bench.py --full --steps 20 --no-cpu-baseline $EXTRA > $O/benchx_$tag.log 2>&1 || exit 1
    fi
    HPE_LIB_VARIANT=$v timeout -k 10 200 python tools/opt_time.py ${OPT_P:-32} 100 1 > $O/opt_$tag.log 2>&1 || exit 1
  done
done
