# kernel-trace statistics of the b = 1 single-graph bench: per-kernel time against the step's wall time
OUT=${OUT:-out}
R=$(pwd); export TMPDIR=/tmp; mkdir -p $R/$OUT
cd /tmp; rm -rf $R/$OUT/prof_b1
(timeout 600 rocprofv3 --kernel-trace --stats -d $R/$OUT/prof_b1 -o bench -- python $R/bench.py --full --batch 1 --graph single --steps 40 --warmup 5 --no-cpu-baseline --no-extras --no-d7 --profile-steps 1 2>&1 | tail -1 | cut -c1-200) > $R/$OUT/r05_b1_rocprof.log 2>&1
cd $R
python tools/kernel_stats.py $OUT/prof_b1 > $OUT/r05_kernel_stats_bench_b1_single.txt 2>&1
find $OUT/prof_b1 -name "*.db" -size +20M -delete
head -24 $OUT/r05_kernel_stats_bench_b1_single.txt | cut -c1-160
