# PMC passes for the dominant kernel (separate runs, --kernel-trace only, as the pool requires)
set -e
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
export OUT=${OUT:-results}   # where the runs write (a folder under the repository root unless an absolute path)
mkdir -p "$OUT"
TAG=${1:-r01}
CFG=${2:-c3}
run() {  # name, counters...
  name=$1; shift
  rm -rf $OUT/pmc_${TAG}_$name
  timeout -k 10 500 rocprofv3 --kernel-trace --pmc "$@" --output-format csv -d $OUT/pmc_${TAG}_$name -- python3 bench.py --config $CFG --steps 1 --warmup 0 --no-cpu-baseline --no-secondary > $OUT/pmc_${TAG}_$name.log 2>&1 || { tail -5 $OUT/pmc_${TAG}_$name.log; exit 1; }
  echo "pass $name done"
}
run sq SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_VALU_MFMA_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_LDS
run grbm GRBM_GUI_ACTIVE SQ_INSTS_VALU_MFMA_MOPS_F64 SQ_INSTS_LDS SQ_INSTS_VMEM_RD
run fetch FETCH_SIZE
run write WRITE_SIZE
python3 tools/pmc_summary.py $OUT $TAG > $OUT/pmc_${TAG}_summary.txt
cat $OUT/pmc_${TAG}_summary.txt
