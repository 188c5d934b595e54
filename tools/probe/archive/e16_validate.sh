# round validation: full GPU suite, the full bench (secondary workloads + cpu_baseline), profiled bench + step by grid
# (bash e16_validate.sh <out dir>; a relative <out dir> is taken from the repository root)
out=${1:?usage: bash e16_validate.sh <out dir>}
cd "$GRAFT_REPO_ROOT"
mkdir -p "$out"
python -m pytest tests -q -x -m gpu 2>&1 | grep -E "passed|failed|error" | tail -3 > "$out/r05_gpu_tests_v3.txt"
cat "$out/r05_gpu_tests_v3.txt"
( time python bench.py --full ) > "$out/r05_bench_v3.json" 2> "$out/r05_bench_v3.err"
tail -3 "$out/r05_bench_v3.err"
cat "$out/r05_bench_v3.json"
bash tools/prof_round.sh r05v3 "$out"
