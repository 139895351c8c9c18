#!/bin/bash
# Runs ON THE GPU BOX: rocprofv3 kernel-trace/stats of the full bench command (bench.py --full), then FETCH_SIZE and
# WRITE_SIZE in separate --pmc passes (MI355X_MICROARCH.md, "rocprofv3 PMC slots": the two do not fit one pass).
# Outputs land in $KNN355_MEASURE_OUT (default measure_out/), where tools/summarize_profiles.py reads them.
# usage: tools/collect_profiles.sh <round-tag>
set -e
TAG=${1:-r01}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${KNN355_MEASURE_OUT:-measure_out}
mkdir -p "$OUT"
rm -rf "$OUT/prof_$TAG" "$OUT/pmc_fetch_$TAG" "$OUT/pmc_write_$TAG"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_$TAG" -o $TAG -- python3 bench.py --full > "$OUT/bench_prof_$TAG.json" 2> "$OUT/bench_prof_$TAG.err"
echo "stats pass ok"
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d "$OUT/pmc_fetch_$TAG" -o f -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu > "$OUT/pmc_fetch_$TAG.json" 2> "$OUT/pmc_fetch_$TAG.err"
echo "fetch pass ok"
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d "$OUT/pmc_write_$TAG" -o w -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu > "$OUT/pmc_write_$TAG.json" 2> "$OUT/pmc_write_$TAG.err"
echo "write pass ok"
