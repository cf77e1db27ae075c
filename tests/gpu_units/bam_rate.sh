#!/bin/bash
# Rates of the BAM path (bam_rate.py) and, in a run of its own, the rocprofv3 kernel statistics of the same script.
# Every step that uses the GPU has its own time limit and the steps are chained: a failure ends the script.
# usage: bam_rate.sh <output directory> [bam_rate.py args...]
out=$1; shift
here=$(cd "$(dirname "$0")" && pwd)
mkdir -p "$out" && rm -rf "$out/bam_rate_prof" &&
timeout -k 10 500 python3 "$here/bam_rate.py" --out "$out/bam_rate.json" "$@" > "$out/bam_rate.log" 2>&1 &&
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/bam_rate_prof" -o bam_rate -- python3 "$here/bam_rate.py" --reps 2 --skip-host "$@" > "$out/bam_rate_prof.log" 2>&1 &&
f=$(find "$out/bam_rate_prof" -name "*kernel_stats.csv" | head -1) && [ -n "$f" ] && cp "$f" "$out/bam_rate_kernel_stats.csv" && rm -rf "$out/bam_rate_prof"
