R=$(pwd); OUT=${OUT:-out}
mkdir -p $OUT; cd /tmp && export TMPDIR=/tmp
rm -rf $R/$OUT/prof_b1
timeout 600 rocprofv3 --kernel-trace -d $R/$OUT/prof_b1 -o b1 -- python $R/bench.py --full --batch 1 --steps 20 --warmup 3 --no-cpu-baseline --profile-steps 1 2>&1 | tail -2
cd $R
python tools/kernel_stats.py $OUT/prof_b1 | head -30
find $OUT/prof_b1 -name "*.db" -size +30M -delete
