#!/bin/bash
# rocprofv3 --kernel-trace --stats of the bench command (headline workload and its --full measurement legs, without
# the CPU baseline and the `also` workloads), summaries copied next to the bench line it printed.
# Usage (on the GPU machine):  bash tools/profile_bench.sh <tag> [<output dir>, default profile_out/]
# -> <output dir>/<tag>_kernel_stats.csv, <output dir>/<tag>_bench_line_under_rocprof.json
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
tag=${1:-r02}
out=$(realpath -m "${2:-$R/profile_out}")
mkdir -p "$out"
cd /tmp && export TMPDIR=/tmp
rm -rf "$out/prof_$tag"
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/prof_$tag" -- \
    python3 $R/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-also \
    > "$out/${tag}_bench_line_under_rocprof.json" 2> "$out/prof_$tag.err"
rc=$?
f=$(ls "$out/prof_$tag"/*/*kernel_stats.csv 2>/dev/null | head -1)
[ -n "$f" ] && cp "$f" "$out/${tag}_kernel_stats.csv" && head -12 "$out/${tag}_kernel_stats.csv" | cut -c1-200
exit $rc
