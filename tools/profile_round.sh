# GPU box: kernel trace of the bench command with its per-kernel timing pass (--full) + one-step table; results under the directory given as $1
cd /tmp; export TMPDIR=/tmp
cd "$GRAFT_REPO_ROOT"
O=${1:?usage: bash tools/profile_round.sh OUT_DIR}
rm -rf $O; mkdir -p $O
rocprofv3 --kernel-trace --stats -d $O/trace -o bench -- python3 bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-excess > $O/bench.log 2>&1
tail -1 $O/bench.log
db=$(ls $O/trace/*.db | head -1)
python3 tools/rocprof_summary.py "$db" $O/kernel_stats.md > /dev/null
python3 tools/rocprof_step.py "$db" > $O/one_step.txt
head -40 $O/one_step.txt
rm -rf $O/trace
