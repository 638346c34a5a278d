#!/bin/bash
# BASELINE.json configs[3] whole on one GPU (scratch tool: the record of profiles/r06_bench_cfg4_full_1gpu.json). Usage: bash tools/dbg/bench_cfg4.sh [out_dir]
OUT=${1:-out}; mkdir -p $OUT
python bench.py --full --workload cfg4 --synth-scaling strong --steps 10 --warmup 2 > $OUT/r06_bench_cfg4_full_1gpu.json 2> $OUT/cfg4.err
cp bench_detail.json $OUT/r06_bench_cfg4_full_1gpu_detail.json
python - $OUT/r06_bench_cfg4_full_1gpu.json <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d["ms_per_step"], d["value"], {k: v for k, v in d.items() if "eval" in k})
PY
