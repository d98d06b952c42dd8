#!/bin/bash
# here, with the outputs of tools/gpu_final.sh <TAG> in $OUT/: copy the files that are to be judged into profiles/
set -eu
OUT=$(mkdir -p "${OUT:-results}" && cd "${OUT:-results}" && pwd)  # where the outputs go (default results/; absolute: some steps run from /tmp)
T=${1:?tag}
latest() { ls -t "$1"/runc/*_kernel_stats.csv | head -1; }
cp $OUT/${T}_pmc_traffic_1080p_nv12.json profiles/pmc_traffic_1080p_nv12_b128.json
cp $OUT/${T}_pmc_traffic_1080p_nv12_full.json profiles/pmc_traffic_1080p_nv12_b128_full.json
cp $OUT/${T}_pmc_traffic_4k_p016.json profiles/pmc_traffic_4k_p016_b48.json
cp "$(latest $OUT/${T}_prof)" profiles/${T}_kernel_stats_1080p_b128.csv
cp "$(latest $OUT/${T}_fused_prof)" profiles/${T}_kernel_stats_1080p_b128_fused.csv
if [ -d $OUT/${T}_alone_prof ]; then cp "$(latest $OUT/${T}_alone_prof)" profiles/${T}_kernel_stats_1080p_b128_alone.csv; fi
cp "$(latest $OUT/${T}_4k_prof)" profiles/${T}_kernel_stats_4k_b48.csv
cp "$(latest $OUT/${T}_fused4k_prof)" profiles/${T}_kernel_stats_4k_b48_fused.csv
cp $OUT/${T}_prof_bench_detail.json profiles/${T}_prof_bench_1080p_detail.json
grep -h '^{"metric"' $OUT/${T}_bench_2ranks_gloo.json | tail -1 > profiles/${T}_bench_2ranks_gloo_one_device.json
cp $OUT/${T}_bench.json $OUT/${T}_bench_detail.json $OUT/${T}_pytest_gpu.log $OUT/${T}_smoke.log $OUT/${T}_env.log profiles/
cp $OUT/${T}_sq_summary.txt profiles/${T}_sq_counters_1080p_b128.txt
cp $OUT/${T}_fused_sq_summary.txt profiles/${T}_sq_counters_1080p_b128_fused.txt
cp $OUT/${T}_b1_sq_summary.txt profiles/${T}_sq_counters_1080p_b1.txt
for f in small_launch_probe deferred_depth pipeline_probe soak_create_destroy cli_1080p cli_4k cli_ab host_fed_ab wr_ceiling fold_ab; do cp $OUT/${T}_$f.log profiles/; done
python3 tools/trace_timeline.py "$(ls -t $OUT/${T}_prof/runc/*_kernel_trace.csv | head -1)" 2 > profiles/${T}_timeline_1080p_b128.txt
ls profiles | grep ${T}
