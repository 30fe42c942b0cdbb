#!/bin/bash
# Round 6 final pass: the JSON device-ingest tests, then the full bench line (default arguments).
set -o pipefail
OUT="${OUT:-out}"; mkdir -p "$OUT"
timeout -k 10 600 python -u -m pytest -x -v --timeout 300 --timeout-method thread tests/test_gpu_json_ingest.py \
  > $OUT/pytest_json.log 2>&1 &&
timeout -k 10 1000 python -u bench.py --full > $OUT/bench_full_r6f.json 2> $OUT/bench_full_r6f.err
rc=$?
tail -3 $OUT/pytest_json.log
tail -c 2500 $OUT/bench_full_r6f.json
exit $rc
