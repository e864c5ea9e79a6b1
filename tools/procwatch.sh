# diagnostic: what processes does bench.py leave or spawn (run on the GPU box)
# Usage: bash tools/procwatch.sh [output directory, default bench_out]
O=${1:-bench_out}; mkdir -p $O
python bench.py --full --steps 3 --warmup 1 --cpu-seconds 1 > $O/pw_bench.log 2>&1 &
B=$!
sleep 12
ps -eo pid,ppid,pgid,stat,etime,comm,args --forest > $O/pw_during.txt
wait $B; echo "bench rc $?" >> $O/pw_during.txt
sleep 1
ps -eo pid,ppid,pgid,stat,etime,comm,args --forest > $O/pw_after.txt
