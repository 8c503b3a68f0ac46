#!/bin/bash
# GPU session: smoke, bench (default, --full), rocprofv3 kernel stats of a short bench,
# then the two HBM PMC passes (FETCH_SIZE / WRITE_SIZE: separate passes, TCC slots).
# Everything is written under $NR_PROFILE_OUT (default: profile_out/ in the repository).
set -o pipefail
cd "${GRAFT_REPO_ROOT:-/root/repo}" || exit 1
OUT="${NR_PROFILE_OUT:-profile_out}"
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1 || { echo "smoke failed"; tail -30 "$OUT/smoke.log"; exit 1; }
tail -2 "$OUT/smoke.log"
timeout -k 10 400 python bench.py --full "$@" > "$OUT/bench.json" 2> "$OUT/bench.err" || { echo "bench failed"; tail -30 "$OUT/bench.err"; exit 1; }
cat "$OUT/bench.json"
rm -rf "$OUT/prof" "$OUT/pmc_fetch" "$OUT/pmc_write"
# the kernel trace runs the driver's bench command (20 timed steps after 5 warm-up steps):
# tools/prof_summary.py ... 20 averages each fused-MLP kernel over its timed launches
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run --output-format csv -- python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline "$@" > "$OUT/prof.log" 2>&1 || { echo "rocprof failed"; tail -30 "$OUT/prof.log"; exit 1; }
timeout -k 10 400 rocprofv3 --pmc FETCH_SIZE -d "$OUT/pmc_fetch" -o run --output-format csv -- python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline "$@" > "$OUT/pmc_fetch.log" 2>&1 || { echo "pmc fetch failed"; tail -30 "$OUT/pmc_fetch.log"; exit 1; }
timeout -k 10 400 rocprofv3 --pmc WRITE_SIZE -d "$OUT/pmc_write" -o run --output-format csv -- python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline "$@" > "$OUT/pmc_write.log" 2>&1 || { echo "pmc write failed"; tail -30 "$OUT/pmc_write.log"; exit 1; }
find "$OUT/prof" "$OUT/pmc_fetch" "$OUT/pmc_write" -name "*.csv" | head -20
