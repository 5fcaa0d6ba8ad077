#!/bin/bash
# Measurement set of one code version on the GPU box, written to $OUT:   OUT=<dir> bash tools/measure.sh <tag> [bench|stats|pmc|calib|mfma ...]
#   bench  : python bench.py --full (K = 20, W = 5)             -> $OUT/<tag>_bench.json
#   stats  : rocprofv3 --kernel-trace --stats of the same command -> $OUT/<tag>_stats/   (copy *kernel_stats.csv to profiles/)
#   pmc    : FETCH_SIZE / WRITE_SIZE, two separate --pmc passes   -> $OUT/pmc_FETCH_SIZE, pmc_WRITE_SIZE  (tools/pmc_traffic.py)
#   calib  : the same two counters on tools/pmc_calib.hip          -> $OUT/calib_*                          (tools/pmc_calib_report.py)
#   mfma   : MFMA / LDS counters                                  -> $OUT/pmc_SQ_*
# Counters are collected in their own runs with --kernel-trace only (pool rule); the program itself follows `--`.
export HPF_ENV_SWITCHES=1
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${OUT:?set OUT to the directory the measurement set is written to}
TAG=${1:-run}; shift
WHAT=${@:-bench stats}
PROF_ARGS="--full --steps 5 --warmup 2 --repeats 1 --cpu-iters 0 --no-finish --no-probe --no-one-group --no-single --sweep-1gpu 0"
for w in $WHAT; do
  case $w in
    bench) timeout -k 10 600 python bench.py --full --steps 20 --warmup 5 > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err; tail -c 400 $OUT/${TAG}_bench.json; echo;;
    stats) rm -rf $OUT/${TAG}_stats; timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_stats -- python3 bench.py $PROF_ARGS > $OUT/${TAG}_stats.log 2>&1; ls $OUT/${TAG}_stats/*/ | head -5;;
    pmc) for c in FETCH_SIZE WRITE_SIZE; do rm -rf $OUT/pmc_$c; timeout -k 10 300 rocprofv3 --pmc $c --kernel-trace --output-format csv -d $OUT/pmc_$c -- python3 bench.py $PROF_ARGS > $OUT/pmc_$c.log 2>&1; done;;
    calib) for c in FETCH_SIZE WRITE_SIZE; do rm -rf $OUT/calib_$c; timeout -k 10 200 rocprofv3 --pmc $c --kernel-trace --output-format csv -d $OUT/calib_$c -- tools/bin/pmc_calib > $OUT/calib_$c.log 2>&1; done; tail -1 $OUT/calib_WRITE_SIZE.log;;
    mfma) for c in "SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES" "SQ_INSTS_VALU_MFMA_F64 SQ_LDS_BANK_CONFLICT SQ_ACTIVE_INST_LDS"; do tag=$(echo $c | cut -d' ' -f1); rm -rf $OUT/pmc_$tag; timeout -k 10 300 rocprofv3 --pmc $c --kernel-trace --output-format csv -d $OUT/pmc_$tag -- python3 bench.py $PROF_ARGS > $OUT/pmc_$tag.log 2>&1; done;;
  esac
done
