#!/bin/bash
# rocprofv3 kernel trace of the bench command with all its legs (python bench.py --full: 2 timed steps + 1 warm-up, secondary
# workloads, VAE decode, cpu_baseline) -> OUT/trace_bench_default_summary.md + the JSON line that run printed.
# usage: tools/trace_bench_default.sh OUT
set -u
out=$(realpath -m "${1:?usage: $0 OUT}")
export TMPDIR=${TMPDIR:-/tmp}
cd "$(dirname "$0")/.." || exit 1
mkdir -p "$out" && rm -rf "$out/trace_bench_default"
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/trace_bench_default" -- python3 bench.py --full > "$out/trace_bench_default.json" 2> "$out/trace_bench_default.err" || { tail -5 "$out/trace_bench_default.err"; exit 1; }
f=$(ls "$out"/trace_bench_default/*/*_kernel_trace.csv | head -1)
python3 tools/summarize_trace.py "$f" "$out/trace_bench_default_summary.md" | head -12
cut -c1-300 "$out/trace_bench_default.json"
