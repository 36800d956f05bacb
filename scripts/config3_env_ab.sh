#!/bin/bash
# Config 3's sampler sweep under two environments on ONE box:
#   bash scripts/config3_env_ab.sh "ENV_A" "ENV_B" [batches=6000,60000,300000] [policies=uniform,recent]
# e.g. "GNNFLOW_SEARCH_GROUP_LARGE=4" "GNNFLOW_SEARCH_GROUP_LARGE=8" (lanes per root, large layers),
#      "GNNFLOW_SAMPLER_HYBRID_SEARCH=1" "GNNFLOW_SAMPLER_HYBRID_SEARCH=0" (the lane-per-root pass).
A=$1; B=$2; BATCHES=${3:-6000,60000,300000}; POL=${4:-uniform,recent}
mkdir -p gpurun_out/c3ab
for side in A B; do
  if [ $side = A ]; then E="$A"; else E="$B"; fi
  echo "== $side [$E]"
  env $E python scripts/config3_bench.py --batches $BATCHES --policies $POL --reps 5 > gpurun_out/c3ab/$side.jsonl 2> gpurun_out/c3ab/$side.err
  python - gpurun_out/c3ab/$side.jsonl <<'PY'
import json, sys
for l in open(sys.argv[1]):
    if l.startswith("{"):
        d = json.loads(l)
        if d.get("sweep") == "config3":
            print(d["policy"], d["batch"], "search %.0f emit %.0f scan %.0f wall %.0f us  search %.0f GB/s emit %.0f GB/s all %.0f" % (
                d["search_us"], d["emit_us"], d["scan_us"], d["wall_us"], d["search_GBps"], d["emit_GBps"], d["all_GBps"]))
PY
done
