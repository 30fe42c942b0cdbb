#!/bin/bash
# The full bench line (driver contract), then the rocprofv3 kernel-trace stats of the headline.
set -u
R="${GRAFT_REPO_ROOT:-$(pwd)}"
cd "$R"; OUT="${OUT:-out}"; mkdir -p "$OUT"
log() { echo "$(date +%T) $*" >> "$R/$OUT/status.log"; }
timeout -k 10 1000 python -u bench.py --full ${BENCH_ARGS:-} > $OUT/bench_full.json 2> $OUT/bench_full.err
rc=$?; log "bench rc=$rc"; tail -5 $OUT/bench_full.err; [ $rc -ne 0 ] && exit $rc
tail -c 3000 $OUT/bench_full.json
exit 0
