#!/bin/bash
# usage: ab.sh "ENV=VAL ..." tag [outdir]   (the full bench line lands in outdir/ab_tag.json; default: a fresh temporary folder)
D=${3:-$(mktemp -d)}
env $1 timeout 200 python bench.py --full --steps 2000 --warmup 200 --no-cpu-baseline > $D/ab_$2.json 2>/dev/null
python - "$D/ab_$2.json" "$2" <<'PY'
import json, sys
d=json.load(open(sys.argv[1]))
print(sys.argv[2], round(d["value"]), "steps/s", round(d["ms_per_step"]*1000,1), "us;", " ".join("%s=%.1f" % (l["name"], l["ms"]*1000) for l in d["step_breakdown"]["launches"]))
PY
