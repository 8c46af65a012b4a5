#!/bin/bash
# Runs ON THE GPU BOX: what the tiled fp16-plane GEMM asks of the L2 under tools/gemm_bench.py on one shape (default: the gated shape
# 16384,1024,1536) -- read requests vector L1 -> L2 (TCP_TCC_READ_REQ: one per 128-byte line touched) and the L2's requests / hits / misses,
# per launch.  TCP and TCC counters in a pass of their own each, counters only with --kernel-trace; the second pass starts only if the
# first one ended well.  A launch needs 384 lines per workgroup and 32-wide K-tile (256 of weight planes, 128 of activations):
# profiles/r10_v3_ab_gemm_wimage.txt.
set -u -o pipefail
OUT=${1:?usage: tools/gemm_l2_pmc.sh OUTPUT_DIR [M,N,K]}
SHAPE=${2:-16384,1024,1536}
mkdir -p $OUT
export TMPDIR=/tmp
pass() { # tag, counters
  local tag=$1; shift
  timeout -k 10 240 rocprofv3 --kernel-trace --pmc "$@" -d $OUT/$tag -o $tag --output-format csv -- python3 tools/gemm_bench.py $SHAPE > $OUT/$tag.out 2> $OUT/$tag.log
}
pass tcp TCP_TCC_READ_REQ_sum TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_LATENCY_sum &&
pass tcc TCC_REQ_sum TCC_HIT_sum TCC_READ_sum TCC_MISS_sum &&
python3 - $OUT <<'PY'
import csv, glob, sys, collections
out = sys.argv[1]
for p in sorted(glob.glob(f"{out}/**/*counter_collection.csv", recursive=True)):
    acc = collections.defaultdict(lambda: [0.0, 0])
    for row in csv.DictReader(open(p)):
        if "gemm_" not in row["Kernel_Name"]: continue
        a = acc[(row["Kernel_Name"][27:60], row["Counter_Name"])]; a[0] += float(row["Counter_Value"]); a[1] += 1
    for k, (v, n) in sorted(acc.items()):
        print(f"{k[0]:34s} {k[1]:32s} per launch {v / n:16.0f}   ({n} launches)")
PY
