# round 4, Winograd-default tree: the tables profiles/r04w_* are made from (run on the GPU box: bash tools/r04w_prof.sh)
set -x
cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
O=gpurun_out/r04w; mkdir -p $O
timeout 900 python bench.py --full > $O/bench_default.json 2> $O/bench_default.err
timeout 300 rocprofv3 --kernel-trace --stats -d $O/bstats -o b --output-format csv -- python bench.py --steps 10 --warmup 2 --no-extras --no-cpu-baseline > $O/bench_profiled.json 2> $O/bench_profiled.err
python tools/kernel_stats_md.py $O/bstats --steps 12 > $O/bench_kernel_stats.md
python tools/step_timeline.py $O/bstats > $O/bench_step_timeline.txt 2>&1
B="python bench.py --steps 4 --warmup 1 --no-extras --no-cpu-baseline"
timeout 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $O/bf -o b --output-format csv -- $B > /dev/null 2>&1
timeout 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $O/bw -o b --output-format csv -- $B > /dev/null 2>&1
python tools/pmc_hbm_md.py $O/bf $O/bw > $O/bench_hbm.md 2>&1
timeout 300 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVE_CYCLES SQ_ACTIVE_INST_ANY SQ_WAIT_INST_ANY SQ_WAIT_ANY --kernel-trace -d $O/bm -o b --output-format csv -- $B > /dev/null 2>&1
python tools/pmc_mfma_md.py $O/bm > $O/bench_mfma.md 2>&1
timeout 300 rocprofv3 --pmc GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES --kernel-trace -d $O/bc -o b --output-format csv -- $B > /dev/null 2>&1
python tools/pmc_clock_md.py $O/bc > $O/bench_clock.md 2>&1
ROUNDS=4 timeout 300 python tools/wino_ab.py > $O/wino_ab.txt 2>&1
VB=64 ROUNDS=3 timeout 300 python tools/wino_ab.py >> $O/wino_ab.txt 2>&1
VB=16 VT=1024 ROUNDS=3 timeout 300 python tools/wino_ab.py >> $O/wino_ab.txt 2>&1
WINO=1 timeout 100 python tools/persist_timing.py > $O/persist_timing_wino.txt 2>&1
WINO=0 timeout 100 python tools/persist_timing.py > $O/persist_timing_direct.txt 2>&1
timeout 300 python tools/latency_bench.py > $O/latency.txt 2>&1
timeout 300 python tools/ragged_bench.py > $O/ragged.txt 2>&1
timeout 900 python tools/config_bench.py > $O/configs.txt 2>&1
CMTTS_FORCE_COLLECTIVE=1 CMTTS_MULTI_EXTRAS=1 timeout 900 python bench.py --full --steps 10 --no-cpu-baseline > $O/bench_collective.json 2> $O/bench_collective.err
rm -rf $O/bstats $O/bf $O/bw $O/bm $O/bc
ls $O
