# GPU box: everything profiles/r05_* holds, in one call (~15 GPU-minutes).  Results under gpurun_out/final5/
cd "$GRAFT_REPO_ROOT"; O=gpurun_out/final5; rm -rf $O; mkdir -p $O
( time timeout 1800 python -m pytest tests -m gpu -q -s 2>&1 ) > $O/gpu_tests.log 2>&1; tail -3 $O/gpu_tests.log
timeout 900 python bench.py --full > $O/bench_c2.json 2> $O/bench_c2.err; cut -c1-300 $O/bench_c2.json
timeout 600 bash tools/profile_round.sh $O/prof_round > $O/profile_round.log 2>&1; cp $O/prof_round/kernel_stats.md $O/prof_round/one_step.txt $O/prof_round/bench.log $O/
cd /tmp; export TMPDIR=/tmp; cd "$GRAFT_REPO_ROOT"
rm -rf $O/fwd_trace; timeout 300 rocprofv3 --kernel-trace --stats -d $O/fwd_trace -o fwd -- python3 bench.py --inference --batch 8 --steps 20 > $O/bench_inf_b8.json 2> $O/bench_inf_b8.err
python3 tools/rocprof_forward.py $(ls $O/fwd_trace/*.db | head -1) > $O/forward_only_kernels.txt 2>&1; rm -rf $O/fwd_trace; head -5 $O/forward_only_kernels.txt
timeout 900 bash tools/pmc_round.sh > $O/pmc_round.log 2>&1; cp gpurun_out/pmc_round/traffic.json $O/pmc_traffic.json
# the floor budget against warm per-launch times (tools/floor_table.py), with the step time bench.py just measured
MS=$(python3 -c "import json; print(json.load(open('$O/bench_c2.json'))['ms_per_step'])")
PYTHONPATH=. timeout 600 python tools/floor_table.py --md $O/floor_budget.md --step-ms $MS > $O/floor_table.log 2>&1; tail -3 $O/floor_table.log
PYTHONPATH=. timeout 300 python tools/bench_narrow.py > $O/bench_narrow.txt 2>&1; tail -8 $O/bench_narrow.txt
timeout 600 python bench.py --full --variant supervised_seg --no-cpu-baseline > $O/bench_c3.json 2> $O/bench_c3.err; cut -c1-200 $O/bench_c3.json
timeout 600 python bench.py --full --batch 4 --height 928 --width 1600 --freeze-seg --variant supervised_seg --steps 10 --warmup 3 --no-cpu-baseline > $O/bench_c4.json 2> $O/bench_c4.err; cut -c1-200 $O/bench_c4.json
timeout 600 python bench.py --full --batch 16 --no-cpu-baseline --no-roofline > $O/bench_c5_b16_bf16.json 2> $O/bench_c5.err; cut -c1-200 $O/bench_c5_b16_bf16.json
timeout 600 python bench.py --full --batch 16 --fp8 --no-cpu-baseline --no-roofline > $O/bench_c5_b16_fp8fwd.json 2>> $O/bench_c5.err; cut -c1-200 $O/bench_c5_b16_fp8fwd.json
timeout 600 python bench.py --full --batch 16 --fp8 --fp8-grad --no-cpu-baseline --no-roofline > $O/bench_c5_b16_fp8fwd_dgrad.json 2>> $O/bench_c5.err; cut -c1-200 $O/bench_c5_b16_fp8fwd_dgrad.json
timeout 600 python bench.py --inference --batch 16 --steps 20 > $O/bench_inf_b16.json 2> $O/bench_inf.err; cut -c1-200 $O/bench_inf_b16.json
timeout 600 python bench.py --inference --fp8 --batch 16 --steps 20 > $O/bench_inf_fp8_b16.json 2>> $O/bench_inf.err; cut -c1-200 $O/bench_inf_fp8_b16.json
timeout 600 python bench.py --inference --batch 1 --height 416 --width 800 --steps 50 > $O/bench_inf_b1.json 2>> $O/bench_inf.err; cut -c1-200 $O/bench_inf_b1.json
CRD_FORCE_DIST=1 timeout 600 python bench.py --full --no-cpu-baseline --no-roofline > $O/bench_c2_forced_dist_1rank.json 2> $O/bench_dist.err; cut -c1-300 $O/bench_c2_forced_dist_1rank.json
# config 5 per kernel: the backward chain of the decoder's two fp8 stages, bf16 against e4m3 data gradients (B = 16)
CRD_CHAIN_BATCH=16 PYTHONPATH=. timeout 600 python tools/chain_table.py bwd 0 40 > $O/chain_c5_bf16.txt 2>&1
CRD_CHAIN_BATCH=16 CRD_CHAIN_FP8=grad PYTHONPATH=. timeout 600 python tools/chain_table.py bwd 0 48 > $O/chain_c5_fp8grad.txt 2>&1; grep -E "fp8|dgrad" $O/chain_c5_fp8grad.txt | head -12
PYTHONPATH=. timeout 900 python tools/train_synth_checkpoint.py 3000 $O/trained_synth.pth > $O/trained_rmse.txt 2>&1; rm -f $O/trained_synth.pth; tail -4 $O/trained_rmse.txt
