#!/bin/bash
# the round's final records: the full bench line (+ detail) and the driver's plain command (scratch tool). Usage: bash tools/dbg/bench_final.sh [out_dir]
OUT=${1:-out}; mkdir -p $OUT
python bench.py --full > $OUT/r06_bench_nf_final.json 2> $OUT/r06_bench_nf_final.err
cp bench_detail.json $OUT/r06_bench_nf_final_detail.json 2>/dev/null
python bench.py --gpus 1 --steps 20 --warmup 5 > $OUT/r06_bench_driver_cmd.json 2>/dev/null
python - $OUT/r06_bench_nf_final.json $OUT/r06_bench_driver_cmd.json <<'PY'
import json, sys
for f in sys.argv[1:]:
    d = json.loads(open(f).read().strip().splitlines()[-1])
    print(f, d["ms_per_step"], d.get("ms_per_step_hip_events"), d["value"], d.get("eval"), (d.get("end_to_end") or {}).get("default"),
          ((d.get("spmm_roofline") or {}).get("ui") or {}).get("ms"), d.get("ml"), d.get("cfg5"), d.get("parity"))
PY
