#!/bin/bash
# Runs ON THE GPU BOX: the step of this tree against the tree in tools/ab/base (git worktree, built there), alternating, same box.
# Prints ms per step, the big kernels and the result hash of each run; PAIRS / STEPS / WARMUP (default 2 / 6 / 2) size the runs,
# DUMP=1 adds one run per tree with --dump-outputs and compares params61.npy byte for byte.  Stops at the first run that fails.
set -u
OUT=gpurun_out/${1:-ab_step}
mkdir -p $OUT
one() { # tag, bench.py, extra args
  local tag=$1 b=$2; shift 2
  local full=$(grep -q -- '"--full"' $b && echo --full)        # a base tree older than --full prints the kernels without it
  timeout -k 10 600 python3 $b --gpus 1 --steps ${STEPS:-6} --warmup ${WARMUP:-2} $full --no-cpu-baseline --no-latency "$@" > $OUT/$tag.json 2> $OUT/$tag.err
  local rc=$?
  if [ $rc != 0 ]; then echo "$tag: bench.py exit $rc"; tail -5 $OUT/$tag.err; exit 1; fi
  python3 - $OUT/$tag.json $tag <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
ks = d.get("kernels", {})
print(sys.argv[2], "ms/step", round(d["ms_per_step"], 1), "sha", d.get("gathered_sha256", "")[:12], {n: round(k["ms"], 1) for n, k in ks.items() if k["ms"] > 5})
PY
}
for rep in $(seq 1 ${PAIRS:-2}); do
  one new$rep bench.py
  one base$rep tools/ab/base/bench.py
done
if [ -n "${DUMP:-}" ]; then
  one new_dump bench.py --dump-outputs $OUT/dump_new
  one base_dump tools/ab/base/bench.py --dump-outputs $OUT/dump_base
  cmp $OUT/dump_new/params61.npy $OUT/dump_base/params61.npy && echo "params61.npy: byte-identical"
fi
