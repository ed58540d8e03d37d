#!/bin/bash
# Kernel trace of the HEADLINE regime (cfg-2 fp32 eval forward, 32 forwards in flight) and, from the same GPU visit, of
# the same forward one at a time (--streams 1); both summarised by tools/rocpd_stats.py, then joined per kernel by
# tools/loaded_vs_single.py (one-at-a-time mean, loaded mean, grid x threads x LDS, share of the loaded GPU-busy time).
# usage: bash tools/profile_loaded_cfg2.sh <tag> [outdir]        (run from anywhere; outdir defaults to build/profile_loaded/)
#   -> <outdir>/loaded_fwd_cfg2_kernel_stats_<tag>.txt, single_fwd_cfg2_kernel_stats_<tag>.txt, loaded_vs_single_<tag>.md
# Every GPU step has its own time limit and the chain stops at the first failure.
set -u
TAG=${1:?usage: profile_loaded_cfg2.sh <tag> [outdir]}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${2:-$ROOT/build/profile_loaded}
mkdir -p "$OUT"
cd "$ROOT" || exit 1

trace() {   # trace <name> <bench args...>
  local name=$1; shift
  rm -rf "$OUT/$name.trace"
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/$name.trace" --output-format rocpd -- \
    python bench.py --gpus 1 --steps 1000 --warmup 50 "$@" > "$OUT/$name.log" 2>&1 || return 1
  local db
  db=$(find "$OUT/$name.trace" -name "*.db" | head -1)
  [ -n "$db" ] || return 1
  python tools/rocpd_stats.py "$db" > "$OUT/$name.txt" || return 1
  rm -rf "$OUT/$name.trace"
  grep -h '"value"' "$OUT/$name.log" | tail -1 | cut -c1-200
}

trace "loaded_fwd_cfg2_kernel_stats_$TAG" &&
trace "single_fwd_cfg2_kernel_stats_$TAG" --streams 1 &&
python tools/loaded_vs_single.py "$OUT/single_fwd_cfg2_kernel_stats_$TAG.txt" "$OUT/loaded_fwd_cfg2_kernel_stats_$TAG.txt" \
  | tee "$OUT/loaded_vs_single_$TAG.md"
