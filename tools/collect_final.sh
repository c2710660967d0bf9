# copy what tools/run_final.sh left under $OUT/ (default results/) into profiles/, in the repository's root: bash tools/collect_final.sh r04
TAG=${1:-r06}
PROFILES=$(pwd)/profiles
cd "${OUT:-results}"
cp final_bench_default.json $PROFILES/${TAG}_bench_default.json
cp final_bench_c2.json $PROFILES/${TAG}_c2_bench.json
cp final_bench_c5.json $PROFILES/${TAG}_c5_bench.json
cp final_bench_c3_fp64_engine.json $PROFILES/${TAG}_c3_bench_fp64_engine.json
cp final_bench_c3_2shards_one_device.json $PROFILES/${TAG}_bench_c3_2shards_one_device.json
cp final_bench_c5_2shards_one_device.json $PROFILES/${TAG}_bench_c5_2shards_one_device.json
cp final_bench_c4_8shards_one_device.json $PROFILES/${TAG}_bench_c4_8shards_one_device_rehearsal.json
cp final_bench_c5_4shards_one_device.json $PROFILES/${TAG}_bench_c5_4shards_one_device_rehearsal.json
cp final_bench_c4_1gpu.json $PROFILES/${TAG}_bench_c4_1gpu.json
cp final_hyperparameter_latency.txt $PROFILES/${TAG}_hyperparameter_latency.txt
[ -f final_ensemble_latency.txt ] && cp final_ensemble_latency.txt $PROFILES/${TAG}_ensemble_latency.txt
cp final_refine_diag_c3.txt $PROFILES/${TAG}_refine_diag_c3.txt
[ -f final_c5_refresh_drift.txt ] && cp final_c5_refresh_drift.txt $PROFILES/${TAG}_c5_refresh_drift.txt
[ -f final_c5_refresh_drift_512.txt ] && cp final_c5_refresh_drift_512.txt $PROFILES/${TAG}_c5_refresh_drift_512.txt
cp final_grad_engine_latency.txt $PROFILES/${TAG}_grad_engine_latency.txt
cp final_oz_soak.txt $PROFILES/${TAG}_oz_soak.txt
[ -f final_c5_cycle.txt ] && cp final_c5_cycle.txt $PROFILES/${TAG}_c5_cycle.txt
for c in c2 c3 c5; do cp final_bench_under_rocprof_$c.json $PROFILES/${TAG}_${c}_bench_under_rocprof.json; cp final_kernel_stats_$c.csv $PROFILES/${TAG}_${c}_kernel_stats.csv; done
cp final_kernel_stats_c3_fp64_engine.csv $PROFILES/${TAG}_c3_kernel_stats_fp64_engine.csv
cp final_pmc_int8_summary.txt $PROFILES/${TAG}_c3_int8_pmc_summary.txt
cp final_pmc_summary.txt $PROFILES/${TAG}_c3_pmc_summary.txt
cp final_c3_pmc_traffic.json $PROFILES/${TAG}_c3_pmc_traffic.json
cp final_c3_int8_pmc_traffic.json $PROFILES/${TAG}_c3_int8_pmc_traffic.json
cp c5_pmc_traffic.json $PROFILES/${TAG}_c5_pmc_traffic.json
cp pmc_c5_fetch_summary.txt $PROFILES/${TAG}_c5_pmc_fetch_summary.txt
cp final_mfma_i8_power_probe.txt $PROFILES/${TAG}_mfma_i8_power_probe.txt
cp final_small_n_latency.txt $PROFILES/${TAG}_small_n_latency.txt
cp final_optimize_acquisition_latency.txt $PROFILES/${TAG}_optimize_acquisition_latency.txt
cp final_c_host_latency.txt $PROFILES/${TAG}_c_host_latency.txt
cp final_fit_times.txt $PROFILES/${TAG}_fit_times.txt
cp fit_trace_summary.txt $PROFILES/${TAG}_fit_trace_summary.txt
cp final_soak.txt $PROFILES/${TAG}_soak.txt
cp final_pytest_gpu.txt $PROFILES/${TAG}_pytest_gpu.txt
cp final_smoke.txt $PROFILES/${TAG}_smoke.txt
cd ..
python tools/update_parity_bounds.py
