#!/bin/bash
# per-launch timeline of one scenario group (rocprofv3 --kernel-trace, HPF_GROUPS=1), written to $OUT:
#   OUT=<dir> bash tools/timeline_run.sh <tag> <scenarios> [ENV=VAL ...]
export HPF_ENV_SWITCHES=1
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${OUT:?set OUT to the directory the trace and timeline are written to}
TAG=$1; S=$2; shift; shift
for kv in "$@"; do export "$kv"; done
export HPF_GROUPS=1
rm -rf $OUT/${TAG}_trace
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $OUT/${TAG}_trace -- python3 bench.py --full --steps 5 --warmup 2 --repeats 1 --cpu-iters 0 --no-finish --no-probe --no-single --sweep-1gpu 0 --scenarios $S > $OUT/${TAG}_trace.log 2>&1
python3 tools/timeline.py $OUT/${TAG}_trace > $OUT/${TAG}_timeline.txt 2>&1
rm -rf $OUT/${TAG}_trace
tail -25 $OUT/${TAG}_timeline.txt
