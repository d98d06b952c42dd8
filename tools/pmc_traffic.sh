#!/bin/bash
# GPU box: HBM traffic of each kernel from the TCC fabric counters, one counter per rocprofv3 pass
# (FETCH_SIZE needs 3 TCC slots, WRITE_SIZE 2: they do not fit one pass; MI355X_MICROARCH.md "rocprofv3 PMC slots").
# The result is stamped with the content hash of csrc/ (tools/parse_pmc.py): bench.py only reports it for that version.
set -u
TAG=${1:-r02}
WL=${2:-1080p_nv12}
EXTRA=${3:-}          # e.g. --full-sums
SUF=${EXTRA:+_full}
OUT=$(mkdir -p "${OUT:-results}" && cd "${OUT:-results}" && pwd)  # where the outputs go (default results/; absolute: some steps run from /tmp)
export TMPDIR=/tmp
R=$(pwd)
cd /tmp
for C in FETCH_SIZE WRITE_SIZE; do
  timeout 600 rocprofv3 --pmc $C --kernel-trace --output-format csv -d $OUT/${TAG}_pmc_${WL}${SUF}_$C -- python3 $R/bench.py --full --workload $WL --steps 3 --warmup 1 --no-cpu-baseline --no-compare --no-extras $EXTRA > $OUT/${TAG}_pmc_$C.log 2>&1
done
cd $R
python3 tools/parse_pmc.py $OUT/${TAG}_pmc_${WL}${SUF}_FETCH_SIZE $OUT/${TAG}_pmc_${WL}${SUF}_WRITE_SIZE $WL > $OUT/${TAG}_pmc_traffic_$WL$SUF.json
cat $OUT/${TAG}_pmc_traffic_$WL$SUF.json
