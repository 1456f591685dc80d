#!/bin/bash
# Round-end style GPU session: parity tests, smoke, bench, rocprofv3 kernel trace of the bench,
# PMC traffic + VALU issue, bench again (reads them).  Summaries -> $PT_OUT/profiles/<tag>_*
# (copy into profiles/).  Stops at the first crash/timeout.
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export TMPDIR=/tmp
export PT_OUT=${PT_OUT:-out}  # logs, raw profiler output and summaries go here (the scripts this one calls share it)
TAG=${1:-r02}
mkdir -p $PT_OUT/profiles
timeout -k 10 900 python -u -m pytest tests -m gpu -q -rP -p no:cacheprovider --timeout 600 --timeout-method thread > $PT_OUT/profiles/${TAG}_pytest_gpu.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -2 $PT_OUT/profiles/${TAG}_pytest_gpu.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 300 python __graft_entry__.py smoke > $PT_OUT/smoke.log 2>&1
rc=$?; echo "smoke rc=$rc"; tail -1 $PT_OUT/smoke.log; if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 600 python bench.py --full > $PT_OUT/bench.log 2>&1
rc=$?; echo "bench rc=$rc"; grep "^{" $PT_OUT/bench.log | cut -c1-200; if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $PT_OUT/bench_kt -o run -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $PT_OUT/bench_kt.log 2>&1
rc=$?; echo "rocprof rc=$rc"; if [ $rc -ne 0 ]; then exit $rc; fi
cp $PT_OUT/bench_kt/run_kernel_stats.csv $PT_OUT/profiles/${TAG}_bench_kernel_stats.csv
grep "^{" $PT_OUT/bench_kt.log > $PT_OUT/profiles/${TAG}_bench_under_rocprof.json || true
# the kernel's busy time from the trace itself (union of its dispatch intervals), for bench.py
cp profiles/trace_union.json $PT_OUT/profiles/trace_union.json 2>/dev/null || true
python3 scripts/trace_union.py $PT_OUT/bench_kt/run_kernel_trace.csv $PT_OUT/profiles/${TAG}_bench_under_rocprof.json \
  $PT_OUT/profiles/trace_union.json > $PT_OUT/profiles/${TAG}_trace_union.log 2>&1
rc=$?; echo "trace union rc=$rc"; grep busy_ms $PT_OUT/profiles/${TAG}_trace_union.log
cp $PT_OUT/profiles/trace_union.json profiles/trace_union.json 2>/dev/null || true
# VALU issue calibration (the traffic summary below applies it)
timeout -k 10 400 bash scripts/calibrate_valu.sh > $PT_OUT/profiles/${TAG}_valu_calibration.log 2>&1
rc=$?; echo "valu calibration rc=$rc"; if [ $rc -ne 0 ]; then exit $rc; fi
cp $PT_OUT/profiles/valu_calibration.json profiles/valu_calibration.json
timeout -k 10 900 bash scripts/collect_traffic.sh
rc=$?; echo "traffic rc=$rc"; if [ $rc -ne 0 ]; then exit $rc; fi
# this box's copy of the tree: let the second bench read the traffic just measured
cp $PT_OUT/profiles/traffic.json profiles/traffic.json
timeout -k 10 300 python bench.py --full > $PT_OUT/bench2.log 2>&1
rc=$?; echo "bench2 rc=$rc"; grep "^{" $PT_OUT/bench2.log | cut -c1-300
grep "^{" $PT_OUT/bench2.log > $PT_OUT/profiles/${TAG}_bench.json || true
cp $PT_OUT/bench.log $PT_OUT/profiles/${TAG}_bench.log
exit $rc
