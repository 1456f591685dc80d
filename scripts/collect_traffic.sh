#!/bin/bash
# HBM traffic and VALU issue of the bench's render kernels from rocprofv3 PMC counters, collected
# as MI355X_MICROARCH.md §HBM prescribes: FETCH_SIZE and WRITE_SIZE in SEPARATE passes (TCC
# slots), no trace domains mixed with --pmc, FETCH_SIZE doubled (gfx950 tallies 128-B requests
# at 64 B), both in KB; a third pass reads SQ_ACTIVE_INST_VALU / GRBM_GUI_ACTIVE for the VALU
# issue fraction.  Writes per-launch figures (keyed by WxHxsppxdepthxworld) to
# $PT_OUT/profiles/traffic.json (copy it into profiles/ locally); raw CSVs stay under
# $PT_OUT/traffic/.  Extra arguments go to bench.py.
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export TMPDIR=/tmp
export PT_OUT=${PT_OUT:-out}  # logs, raw profiler output and summaries go here (the scripts this one calls share it)
OUT=$PT_OUT/traffic
rm -rf $OUT
mkdir -p $OUT
ARGS="--full --steps 2 --warmup 0 --no-cpu-baseline $*"
timeout -k 10 600 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/fetch -o run -- python3 bench.py $ARGS > $OUT/fetch.log 2>&1 || exit $?
timeout -k 10 600 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/write -o run -- python3 bench.py $ARGS > $OUT/write.log 2>&1 || exit $?
timeout -k 10 600 rocprofv3 --pmc SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_THREAD_CYCLES_VALU SQ_WAVE_CYCLES SQ_WAVES GRBM_GUI_ACTIVE \
  --output-format csv -d $OUT/valu -o run -- python3 bench.py $ARGS > $OUT/valu.log 2>&1 || exit $?
mkdir -p $PT_OUT/profiles
cp profiles/traffic.json $PT_OUT/profiles/traffic.json 2>/dev/null || true
python3 scripts/summarize_traffic.py $PT_OUT/profiles/traffic.json
