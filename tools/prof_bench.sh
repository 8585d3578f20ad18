# Full GPU test suite, the default full bench line, and the rocprofv3 kernel statistics of the
# same bench command (profiles/ copies are made by hand afterwards).
# Usage: bash tools/prof_bench.sh <output dir>
set -e
export TMPDIR=/tmp
OUT=${1:?usage: bash tools/prof_bench.sh <output dir>}
mkdir -p "$OUT"
timeout -k 10 600 python -u -m pytest tests -m gpu -q -x --timeout 120 --timeout-method thread > "$OUT/t_all.log" 2>&1
timeout -k 10 400 python -u bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err"
rm -rf "$OUT/prof"
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -o run -- python3 -u bench.py --full --no-cpu --no-llama > "$OUT/bench_prof.json" 2> "$OUT/bench_prof.err"
