#!/bin/bash
# tools/mid_check.sh [tag] -- the whole GPU suite, then the full bench.py line, summarised; results under $OUT (default out/)
cd "$(dirname "$0")/.."
TAG=${1:-mid}
OUT=${OUT:-out}
mkdir -p "$OUT"
python -m pytest tests -m gpu -x -q > "$OUT/${TAG}_tests.txt" 2>&1
rc=$?
tail -3 "$OUT/${TAG}_tests.txt"
[ $rc -ne 0 ] && exit $rc
python bench.py --full > "$OUT/${TAG}_bench.json" 2> "$OUT/${TAG}_bench.err" || { tail -5 "$OUT/${TAG}_bench.err"; exit 1; }
python tools/bench_brief.py "$OUT/${TAG}_bench.json"
