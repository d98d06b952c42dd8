#!/bin/bash
# Runs on a GPU box: GPU tests, smoke, bench --full (the compact line on stdout, the full record with every leg in <TAG>_bench_detail.json),
# the 2-rank bench over gloo, rocprof kernel-trace. Outputs -> $OUT/ (set OUT to choose the folder)
set -u
R=$(pwd)
OUT=$(mkdir -p "${OUT:-results}" && cd "${OUT:-results}" && pwd)  # where the outputs go (default results/; absolute: some steps run from /tmp)
export TMPDIR=/tmp
TAG=${1:-r02}
echo "== rocminfo" > $OUT/${TAG}_env.log
(rocminfo | grep -E "Marketing Name|gfx" | head -6; nproc; lscpu | grep "Model name") >> $OUT/${TAG}_env.log 2>&1
echo "== pytest -m gpu"
timeout 1500 python -m pytest tests -x -q -m gpu 2>&1 | tail -25 | tee $OUT/${TAG}_pytest_gpu.log
echo "== smoke"
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -5 | tee $OUT/${TAG}_smoke.log
echo "== bench --full"
( time timeout 900 python bench.py --full --detail-file $OUT/${TAG}_bench_detail.json ) 2>&1 | tail -8 | tee $OUT/${TAG}_bench.json
echo "== bench --gpus 2 over gloo on one device"
TM_BENCH_BACKEND=gloo timeout 900 python bench.py --full --gpus 2 --steps 10 --warmup 2 --no-extras --detail-file $OUT/${TAG}_bench_2ranks_gloo_detail.json 2>&1 | tail -3 | tee $OUT/${TAG}_bench_2ranks_gloo.json
echo "== rocprof"
cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_prof -- python3 $R/bench.py --full --steps 20 --warmup 2 --no-cpu-baseline --no-compare --no-extras --detail-file $OUT/${TAG}_prof_bench_detail.json > $OUT/${TAG}_prof_bench.log 2>&1
cd $R
for f in $(find $OUT/${TAG}_prof -name "*kernel_stats*.csv" | head -1); do head -12 $f; done
