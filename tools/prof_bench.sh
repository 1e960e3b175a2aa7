#!/bin/bash
# Round profile of the default workload's --full bench line (run on the GPU box): kernel-trace stats,
# then separate FETCH_SIZE / WRITE_SIZE passes for the HBM traffic of the dominant kernels.
#   bash tools/prof_bench.sh [tag]      -> $PNR_PROF_OUT/prof_<tag>/...   (default prof_out/)
TAG=${1:-bench}
OUT=${PNR_PROF_OUT:-prof_out}
cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
set -e
mkdir -p $OUT
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o bench -- \
  python3 bench.py --steps 3 --warmup 1 --full --no-cpu-baseline > $OUT/prof_${TAG}.log 2>&1
for C in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 400 rocprofv3 --kernel-trace --pmc $C --output-format csv -d $OUT/prof_${TAG}_traffic -o $C -- \
    python3 bench.py --steps 1 --warmup 0 --full --no-cpu-baseline > $OUT/prof_${TAG}_$C.log 2>&1
done
echo PROF_DONE
