#!/bin/bash
# Runs ON THE GPU BOX: the step with the library in the tree against tools/diag/libdvq_hip_diag.so (an older build put there by hand),
# alternating, same box.  Prints ms per step, the big kernels and the result hash of each run.
set -u
OUT=gpurun_out/${1:-ab}
mkdir -p $OUT
for rep in 1 2; do
  for v in new old; do
    if [ $v = old ]; then export DVQ_DIAG_LIB=1; else unset DVQ_DIAG_LIB; fi
    timeout 600 python3 bench.py --gpus 1 --steps 6 --warmup 2 --full --no-cpu-baseline --no-latency > $OUT/$v$rep.json 2> $OUT/$v$rep.err
    python3 - $OUT/$v$rep.json $v$rep <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
ks = d.get("kernels", {})
print(sys.argv[2], "ms/step", round(d["ms_per_step"], 1), "sha", d.get("gathered_sha256", "")[:12], {n: round(k["ms"], 1) for n, k in ks.items() if k["ms"] > 5})
PY
  done
done
