# one driving-fp16 line per walker count of the 4x4 / stride 2 weight gradient:  scratch/k4_walkers.sh <output directory>
out=$1; mkdir -p $out
for w in 384 512 768 256; do
  for i in 1 2; do
    SRGAN_H_K4_WALKERS=$w python bench.py --full --workload driving-fp16 --steps 100 --warmup 5 --no-secondary --no-cpu-baseline 2>/dev/null | grep '^{' | tail -1 > $out/w${w}_$i.json
  done
done
python - <<PY
import json, glob, os
for path in sorted(glob.glob("$out/*.json")):
    d = json.load(open(path)); r = d["roofline"]
    print(os.path.basename(path), round(d["value"], 1), round(d["ms_per_step"], 2), round(r["frac"], 4), round(r["kernel_ms_per_step"], 2))
PY
