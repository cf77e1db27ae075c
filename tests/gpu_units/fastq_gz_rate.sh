#!/bin/bash
# Rates of compressed FASTQ in (fastq_gz_rate.py) and, in a run of its own, the rocprofv3 kernel statistics of the same script.
# Every step that uses the GPU has its own time limit and the steps are chained: a failure ends the script.
# usage: fastq_gz_rate.sh <output directory> [fastq_gz_rate.py args, e.g. --files --parent-lib <libbwamem_hip.so of the parent commit>]
out=$1; shift
here=$(cd "$(dirname "$0")" && pwd)
mkdir -p "$out" && rm -rf "$out/fastq_gz_rate_prof" &&
timeout -k 10 560 python3 "$here/fastq_gz_rate.py" --out "$out/fastq_gz_rate_2000000reads.json" "$@" > "$out/fastq_gz_rate.log" 2>&1 &&
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/fastq_gz_rate_prof" -o fastq_gz_rate -- python3 "$here/fastq_gz_rate.py" --reps 1 --pairs 0 > "$out/fastq_gz_rate_prof.log" 2>&1 &&
f=$(find "$out/fastq_gz_rate_prof" -name "*kernel_stats.csv" | head -1) && [ -n "$f" ] && cp "$f" "$out/fastq_gz_rate_kernel_stats.csv" && rm -rf "$out/fastq_gz_rate_prof"
