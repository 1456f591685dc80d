#!/bin/bash
# BASELINE.json configs[2..3] at their stated spp (depth 16, the reference default) plus the fast
# SAH tree of the same scenes: one bench line each -> $PT_OUT/profiles/<TAG>_configs.jsonl
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export TMPDIR=/tmp
export PT_OUT=${PT_OUT:-out}  # logs, raw profiler output and summaries go here (the scripts this one calls share it)
TAG=${1:-r02}
OUT=$PT_OUT/profiles/${TAG}_configs.jsonl
mkdir -p $PT_OUT/profiles
: > $OUT
run() {
  timeout -k 10 600 python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline "$@" > $PT_OUT/cfg.log 2>&1
  rc=$?; echo "config $* rc=$rc"; [ $rc -eq 0 ] || exit $rc
  grep -h '^{' $PT_OUT/cfg.log >> $OUT
}
run --scene CornellBox-Mirror --spp 1024 --depth 16
run --scene CornellBox-Glossy --spp 1024 --depth 16
run --scene CornellBox-Glossy --spp 1024 --depth 16 --bvh sah
run --scene MedievalBoat --width 1920 --height 1080 --spp 512 --depth 16
run --scene MedievalBoat --width 1920 --height 1080 --spp 512 --depth 16 --bvh sah
python3 - "$OUT" <<'PY'
import json, sys
for l in open(sys.argv[1]):
    d = json.loads(l); r = d["roofline"]
    print(d["metric"], d["config"]["bvh"], d["value"], "Msamples/s", r["kernel"], "frac", r["frac"])
PY
