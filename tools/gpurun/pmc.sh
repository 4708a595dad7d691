OUT=${OUT:-out}; mkdir -p "$OUT"
R=$(pwd)
cd /tmp && export TMPDIR=/tmp
CMD="python $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --profile-steps 1"
for c in FETCH_SIZE WRITE_SIZE "SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES GRBM_GUI_ACTIVE" "SQ_INSTS_VALU_MFMA_MOPS_F32 SQ_WAVES SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE"; do
  tag=$(echo $c | tr ' ' '_' | cut -c1-40)
  timeout 600 rocprofv3 --kernel-trace --pmc $c --output-format csv -d $R/$OUT/pmc_$tag -o pmc -- $CMD > $R/$OUT/pmc_$tag.log 2>&1
  ls $R/$OUT/pmc_$tag | head -5
done
rocprofv3 -L 2>/dev/null | grep -i -E "mfma|FETCH_SIZE|WRITE_SIZE|TCC_EA0_RDREQ|TCC_HIT" | head -30 > $R/$OUT/counters_list.txt
