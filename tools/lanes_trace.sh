#!/bin/bash
# GPU box: kernel timelines of the 128-pair step with an RCCL communicator created BEFORE the engine (TM_BENCH_FORCE_DIST=1: a one-rank
# process group, what bench.py --gpus N does on every rank), with and without the hardware-queue lanes -> $OUT/<TAG>_lanes{1,0}_timeline.txt
set -u
OUT=$(mkdir -p "${OUT:-results}" && cd "${OUT:-results}" && pwd)  # where the outputs go (default results/; absolute: some steps run from /tmp)
TAG=${1:-r06y15}
export TMPDIR=/tmp RANK=0 LOCAL_RANK=0 WORLD_SIZE=1 MASTER_ADDR=127.0.0.1 MASTER_PORT=29544 TM_BENCH_FORCE_DIST=1
R=$(pwd)
for q in 1 0; do
  export TM_QUEUE_LANES=$q
  cd /tmp && timeout 300 rocprofv3 --kernel-trace --output-format csv -d $OUT/${TAG}_lanes${q}_prof -- python3 $R/bench.py --full --steps 6 --warmup 2 --no-cpu-baseline --no-compare --no-extras > $OUT/${TAG}_lanes${q}_bench.log 2>&1
  cd $R
  python3 tools/trace_timeline.py "$(ls -t $OUT/${TAG}_lanes${q}_prof/*/*_kernel_trace.csv | head -1)" 2 > $OUT/${TAG}_lanes${q}_timeline.txt
  grep '^{' $OUT/${TAG}_lanes${q}_bench.log | python3 -c "import sys,json; d=json.loads(sys.stdin.read()); print('TM_QUEUE_LANES=$q', d['value'], d['summary'].get('stage_ms'))"
done
