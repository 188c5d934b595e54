#!/bin/bash
# Round profile of the headline bench on an MI355X: bash tools/prof_round.sh <tag> <out dir>   (writes <out dir>/<tag>_*;
# a relative <out dir> is taken from the repository root)
#  (1) rocprofv3 --kernel-trace --stats of the bench command (graph replays, three streams) -> kernel stats CSV
#  (2) one-stream launch-by-launch trace of 6 steps -> per (kernel, grid) table of the steady state
tag=$1
out=${2:?usage: bash tools/prof_round.sh <tag> <out dir>}
cd /tmp && export TMPDIR=/tmp
cd "$GRAFT_REPO_ROOT"
mkdir -p "$out"
rm -rf /tmp/pr1 /tmp/pr2
timeout 900 rocprofv3 --kernel-trace --stats -d /tmp/pr1 -o p -f csv -- python3 bench.py --full --no-secondary --no-cpu-baseline > "$out/${tag}_bench_profiled.json" 2> /tmp/pr1.log
cp "$(find /tmp/pr1 -name '*kernel_stats.csv' | head -1)" "$out/${tag}_bench_kernel_stats.csv"
GS_SIDE_STREAM=0 GS_STEP_GRAPH=0 timeout 900 rocprofv3 --kernel-trace -d /tmp/pr2 -o p -- python3 bench.py --steps 4 --warmup 2 --no-secondary --no-cpu-baseline --no-kernel-timing > /dev/null 2> /tmp/pr2.log
python tools/prof_by_grid.py "$(find /tmp/pr2 -name '*.db' | head -1)" --of 6 --steps 3 --top 70 > "$out/${tag}_step_by_grid.txt"
head -5 "$out/${tag}_step_by_grid.txt"
