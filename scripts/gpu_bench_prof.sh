#!/bin/bash
# optional pytest -k subset, then the full bench (JSON line with every extra record) and a rocprofv3
# kernel-trace/stats run of one clip.  usage: scripts/gpu_bench_prof.sh <tag> [pytest -k expr]
# logs and profiles go to $OUT_DIR (default bench_out/)
set -u
out=${OUT_DIR:-bench_out}
mkdir -p "$out"
tag=${1:-x}
if [ -n "${2:-}" ]; then
  scripts/gpustep.sh 900 "$out/t_$tag.log" python -u -m pytest tests -m gpu -v -rP --maxfail 3 --timeout 600 --timeout-method thread -k "$2"
  rc=$?; echo "tests rc=$rc"; tail -4 "$out/t_$tag.log"; [ $rc -ne 0 ] && exit $rc
fi
scripts/gpustep.sh 900 "$out/bench_$tag.log" python -u bench.py --full; rc=$?; echo "bench rc=$rc"
tail -2 "$out/bench_$tag.log"; [ $rc -ne 0 ] && exit $rc
export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/prof_$tag" -o run -- python bench.py --steps 1 --warmup 0 > "$out/prof_$tag.log" 2>&1
rc=$?; echo "prof rc=$rc"; exit $rc
