#!/bin/bash
# One rocprofv3 hardware-counter pass of bench.py (counters in their own run: --kernel-trace + --pmc only).
#   bash tools/pmc.sh <tag> "<COUNTER ...>" <bench args...>   ->   $OUT/<tag>.db (rocpd database; OUT defaults to profile_out/ in the repository)
set -e
TAG=$1; CTRS=$2; shift 2
REPO=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "${OUT:=$REPO/profile_out}"; OUT=$(cd "$OUT" && pwd)
cd /tmp && export TMPDIR=/tmp
P=$OUT/pmc_$TAG
rm -rf "$P"; mkdir -p "$P"
cd "$REPO"
rocprofv3 --kernel-trace --pmc $CTRS -d "$P" -o run -- python3 bench.py "$@" --cpu-budget 0 --no-roofline --no-epoch --no-configs2 --no-trials > "$P/bench.log" 2>&1 || { tail -5 "$P/bench.log"; exit 1; }
db=$(find "$P" -name '*_results.db' | head -1)
cp "$db" "$OUT/${TAG}.db"
rm -rf "$P"
ls -la "$OUT/${TAG}.db"
