#!/bin/bash
# rocprofv3 kernel-trace summary of bench.py on an MI355X; run as:  bash tools/profile.sh <tag> <bench args...>
# writes $OUT/<tag>_kernel_stats.csv (per-kernel calls / total / average, from the rocpd database through
# tools/kstats.py) and $OUT/<tag>_bench.json (the bench line of the profiled run); OUT defaults to profile_out/ in the repository
set -e
TAG=$1; shift
REPO=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "${OUT:=$REPO/profile_out}"; OUT=$(cd "$OUT" && pwd)
cd /tmp && export TMPDIR=/tmp
P=$OUT/prof_$TAG
rm -rf "$P"; mkdir -p "$P"
cd "$REPO"
rocprofv3 --kernel-trace --stats -d "$P" -o run -- python3 bench.py "$@" --cpu-budget 0 --no-roofline --no-epoch --no-configs2 --no-trials > "$P/bench.log" 2>&1
db=$(find "$P" -name '*_results.db' | head -1)
python3 tools/kstats.py "$db" "$OUT/${TAG}_kernel_stats.csv"
grep '^{' "$P/bench.log" > "$OUT/${TAG}_bench.json" || true
rm -rf "$P"
head -12 "$OUT/${TAG}_kernel_stats.csv" | cut -c1-150
