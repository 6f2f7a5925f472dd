#!/bin/bash
# rocprofv3 kernel trace + stats of the full bench command, the by-grid split, the
# bench-vs-trace cross-check of the level kernel's launch times and the gap timeline, then
# (optionally) the PMC passes of tools/pmc_r03.sh for the roofline fields.
#   usage (GPU box): bash tools/run_prof.sh <tag> [pmc shapes...]     -> $DM_PROF_OUT/<tag>_*
#   (DM_PROF_OUT: output directory, default prof_out/ in the repository root)
set -euo pipefail
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
T=$1; shift
O=${DM_PROF_OUT:-$R/prof_out}
mkdir -p "$O"
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/${T}_prof -o run -- python3 $R/bench.py --full --no-cpu-baseline > $O/${T}_bench_profiled.json 2> $O/${T}_bench_profiled.err
cd $R
python3 tools/kstats.py $O/${T}_prof > $O/${T}_kernel_stats_by_grid.csv
python3 tools/level_launches.py $O/${T}_prof $O/${T}_bench_profiled.json "$T" > $O/${T}_level_kernel_launches.txt
python3 tools/gap_trace.py $O/${T}_prof > $O/${T}_gaps.txt
cp $(find $O/${T}_prof -name '*kernel_stats.csv' | head -1) $O/${T}_kernel_stats.csv
rm -rf $O/${T}_prof
if [ $# -gt 0 ]; then bash tools/pmc_r03.sh $T "$@"; fi
