# Round-4 profile collection (run on the GPU box): GPU tests, rocprofv3 kernel stats of the bench step and of the other SURVEY 8(d)
# workloads, PMC passes (HBM bytes, SQ stalls) on one B=32 training render, SQ counters + launch chains of the CLIP tower, the GEMM lab,
# the 1-rank exchange-schedule timing, the full default bench line.  Only the small summaries are kept (gpurun_out/r04_profiles -> profiles/r04_*).
export MIOPEN_LOG_LEVEL=1
R=$PWD
O=$R/gpurun_out/r04_profiles
mkdir -p $O
timeout 1500 python -m pytest tests -m gpu -q -p no:cacheprovider --timeout 1200 2>&1 | grep -E "passed|failed|Error" | tail -3 > $O/gputest.log
timeout 300 tools/micro/gemm_lab.bin > $O/gemm_lab_final.txt 2>&1
timeout 600 python tools/overlap_1rank.py 100 32 2>&1 | grep -E "^\(" > $O/overlap_1rank.txt
cd /tmp && export TMPDIR=/tmp
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/p_bench -o bench -- python $R/bench.py --no-workloads --no-cpu-baseline --no-alt --sustained 0 --steps 10 > $O/bench_under_rocprof.log 2>&1
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/p_wl -o wl -- python $R/bench.py --workloads-only --no-cpu-baseline > $O/workloads_under_rocprof.log 2>&1
timeout 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d /tmp/p_fetch -o f -- python $R/tools/perf_render.py --B 32 --iters 1 --yaml $R/options/pix3d/config.yaml > /dev/null 2>&1
timeout 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d /tmp/p_write -o w -- python $R/tools/perf_render.py --B 32 --iters 1 --yaml $R/options/pix3d/config.yaml > /dev/null 2>&1
timeout 300 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_LDS_BANK_CONFLICT SQ_INSTS_VALU --output-format csv -d /tmp/p_sq -o s -- python $R/tools/perf_render.py --B 32 --iters 1 --yaml $R/options/pix3d/config.yaml > /dev/null 2>&1
for W in "32 B/32" "256 B/32" "32 L/14"; do
  tag=$(echo $W | tr ' /' '__')
  timeout 300 rocprofv3 --kernel-trace --output-format csv -d /tmp/kt_$tag -o k -- python $R/tools/perf_clip.py $W > /dev/null 2>&1
  n=90; [ "$W" = "32 L/14" ] && n=180
  python $R/tools/trace_gaps.py $(find /tmp/kt_$tag -name "*kernel_trace.csv" | head -1) $n -q > $O/clip_gaps_$tag.txt 2>&1
done
cd $R
cp $(find /tmp/p_bench -name "*kernel_stats.csv" | head -1) $O/bench_bs32_kernel_stats.csv
cp $(find /tmp/p_wl -name "*kernel_stats.csv" | head -1) $O/workloads_kernel_stats.csv
python tools/summarize_prof.py $O/bench_bs32_kernel_stats.csv 45 > $O/bench_bs32_summary.txt
python tools/summarize_prof.py $O/workloads_kernel_stats.csv 30 > $O/workloads_summary.txt
python tools/summarize_pmc.py $(find /tmp/p_fetch -name "*counter_collection.csv" | head -1) > $O/pmc_fetch_size.txt
python tools/summarize_pmc.py $(find /tmp/p_write -name "*counter_collection.csv" | head -1) > $O/pmc_write_size.txt
python tools/summarize_pmc.py $(find /tmp/p_sq -name "*counter_collection.csv" | head -1) > $O/pmc_sq_stalls.txt
grep "^{" $O/bench_under_rocprof.log | tail -1 > $O/bench_line_under_rocprof.json; rm -f $O/bench_under_rocprof.log
grep "^{" $O/workloads_under_rocprof.log | tail -1 > $O/workloads_line_under_rocprof.json; rm -f $O/workloads_under_rocprof.log
bash tools/prof_clip_pmc.sh > /dev/null 2>&1; cp gpurun_out/clip_pmc/pmc_clip_sq.txt $O/pmc_clip_sq.txt 2>/dev/null
timeout 900 python bench.py --full > $O/bench_full.log 2>&1
grep "^{" $O/bench_full.log | tail -1 > $O/bench_line.json; rm -f $O/bench_full.log
cat $O/gputest.log; cat $O/overlap_1rank.txt; head -c 600 $O/bench_line.json; du -sh $O
