# A/B two in-tree builds over three bench configs: default (N = 250), full cloud, 4096 x 40.
# Usage (on the box): bash tools/gpu_ab3.sh [libA.so] [rounds]
# Logs go to $AB_OUT (default bench_out/ab); tools/ab_show.py summarises them.
set -o pipefail
A=${1:-libhpe_base.so}
R=${2:-2}
O=${AB_OUT:-bench_out/ab}
rm -rf $O; mkdir -p $O
for r in $(seq 1 $R); do
  for v in "$A" libhpe.so; do
    tag=$(basename $v .so)_$r
    HPE_LIB_VARIANT=$v timeout -k 10 200 python bench.py --full --steps 40 --no-cpu-baseline > $O/bench_$tag.log 2>&1 || exit 1
    HPE_LIB_VARIANT=$v timeout -k 10 200 python bench.py --full --steps 10 --full-cloud --no-cpu-baseline > $O/full_$tag.log 2>&1 || exit 1
    HPE_LIB_VARIANT=$v timeout -k 10 200 python bench.py --full --steps 10 --particles 4096 --generations 40 --no-cpu-baseline > $O/p4096_$tag.log 2>&1 || exit 1
  done
done
