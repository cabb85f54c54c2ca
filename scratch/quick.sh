#!/bin/bash
# one bench line + the per-kernel table of its roofline leg: scratch/quick.sh <output directory> [bench arguments]
out=$1; shift
mkdir -p $out
timeout 600 python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --shape-report $out/shapes.txt "$@" > $out/bench.json 2> $out/bench.err
python scratch/shapes.py $out/shapes.txt > $out/table.md 2>&1
head -${QUICK_LINES:-17} $out/table.md
python - <<PY
import json
d = json.loads([l for l in open("$out/bench.json") if l.startswith("{")][-1])
r = d.get("roofline", {})
print("images/s %.2f  ms %.2f  frac %.4f  step_frac %.4f  launches %s" % (d["value"], d["ms_per_step"], r.get("frac", 0), r.get("step_frac_executed") or 0, r.get("launches")))
PY
