# PMC passes over the bench (one counter group per run; no trace domains besides kernel-trace).  Run from the repository
# root; output under $SLAM_PROFILE_OUT (default profile_out/)/pmc.
ROOT=$(pwd)
OUT=$(realpath -m ${SLAM_PROFILE_OUT:-profile_out})/pmc
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
rocprofv3 -L > $OUT/counters_list.txt 2>&1
run() {  # name, counters...
  name=$1; shift
  timeout -k 10 300 rocprofv3 --kernel-trace --pmc "$@" --output-format csv -d $OUT/$name -o p -- python3 $ROOT/bench.py --full --steps 6 --warmup 2 --no-cpu-baseline --no-pmc --no-configs > $OUT/$name.log 2>&1
  echo "$name exit $?" >> $OUT/summary.log
}
run sq1 SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU
run sq2 SQ_INSTS_MFMA SQ_INST_CYCLES_VMEM SQ_WAIT_INST_LDS SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_LDS SQ_ACTIVE_INST_VMEM
run fetch FETCH_SIZE
run write WRITE_SIZE
run tcc TCC_HIT_sum TCC_MISS_sum TCC_EA0_RDREQ_sum TCC_EA0_WRREQ_sum
run grbm GRBM_GUI_ACTIVE GRBM_COUNT
cat $OUT/summary.log
