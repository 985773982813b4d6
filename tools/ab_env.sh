#!/bin/bash
# same-device A/B of engine-level switches on the bench workload: tools/ab_env.sh "NAME=ENV=VAL ..." ...   (interleaved, two rounds)
# e.g. tools/ab_env.sh "fold=" "nofold=DD_NO_LN_FOLD=1" "norows=DD_NO_LN_ROWSTATS=1"   -> $OUT/ab_<name>.json, ops_<name>.csv (OUT: default ./ab)
OUT=$(realpath -m "${OUT:-ab}"); mkdir -p "$OUT"
for round in 1 2; do
  for spec in "$@"; do
    name=${spec%%=*}; envs=${spec#*=}
    env $envs DD_PROFILE_DUMP=$OUT/ops_$name.csv timeout -k 10 600 python bench.py --steps 2 --warmup 1 --full --no_cpu_baseline --no_cli --no_strength1 2>$OUT/ab_$name.err | tail -1 > $OUT/ab_$name.json || exit 1
    python - "$OUT/ab_$name.json" "$name" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read())
print(sys.argv[2], "img/s %.3f" % d["value"], "ms/step %.1f" % d["ms_per_step"], d["roofline"].get("family_ms"))
PY
  done
done
