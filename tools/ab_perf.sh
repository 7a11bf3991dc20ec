#!/bin/bash
# GPU box: A/B of environment settings inside ONE run (box-to-box spread is +-3 %): two builds of the library (OCTSEG_LIB=path, see the
# Makefile's B= / OUT= / EXTRA=) or one of the remaining switches.  usage: ab_perf.sh "<env A>" "<env B>" [more...]
out=${OUT:-out}; mkdir -p $out
i=0
for e in "$@"; do
  i=$((i+1))
  env $e OCTSEG_PROFILE_DUMP=$out/layers_ab$i.csv python bench.py --full --steps 4 --warmup 2 --no-cpu-baseline > $out/ab$i.json 2>/dev/null
  echo "== [$e]"; python - <<PY
import json
d = json.load(open('$out/ab$i.json')); r = d['roofline']
print('frames/s', d['value'], 'mfma alone', r['kernel_ms_per_step'], {k: v['ms_per_step'] for k, v in r['by_class'].items()})
PY
  python tools/group_layers.py $out/layers_ab$i.csv 2 | grep -E "decoder 3x3|encoder 3x3 .*(fwd|dgrad)"
done
