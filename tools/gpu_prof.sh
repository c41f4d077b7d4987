#!/bin/bash
# rocprofv3 kernel-trace summary of bench.py (tag = $1; results under $OUT_DIR/<tag>, default bench_out/<tag>)
set -o pipefail
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
TAG=${1:-prof}
OUT=${OUT_DIR:-bench_out}/$TAG
mkdir -p $OUT
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT -o run --output-format csv -- python -u bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $OUT/bench.log 2>&1
rc=$?
tail -3 $OUT/bench.log
find $OUT -name "*stats*" | head
exit $rc
