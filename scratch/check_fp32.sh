#!/bin/bash
# fp32 parity suites + the headline twice + 224 (after a change to the fp32 kernels):  scratch/check_fp32.sh <output directory>
out=$1; mkdir -p $out
python -m pytest tests/test_ops_gpu.py tests/test_steps_gpu.py tests/test_determinism_gpu.py tests/test_grouped_weight_gradients_gpu.py -x -q > $out/tests.log 2>&1; tail -3 $out/tests.log
for i in 1 2; do python bench.py --full --steps 20 --warmup 5 --no-secondary --no-cpu-baseline 2>/dev/null | grep "^{" | tail -1 > $out/bench$i.json; done
python bench.py --full --steps 20 --warmup 5 --no-secondary --no-cpu-baseline --image-size 224 2>/dev/null | grep "^{" | tail -1 > $out/bench224.json
python - <<PY
import json
for n in ["bench1", "bench2", "bench224"]:
    d = json.load(open("$out/%s.json" % n)); r = d["roofline"]
    print(n, round(d["value"], 2), round(d["ms_per_step"], 2), round(r["frac"], 4), round(r["kernel_ms_per_step"], 1))
PY
