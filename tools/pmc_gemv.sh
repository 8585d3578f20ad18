# HBM traffic of the stacked config-2 GEMV kernel: two rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE),
# each its own run, then tools/pmc_traffic.py -> <output dir>/traffic_q4_0_gemv.json.
# Usage: bash tools/pmc_gemv.sh <output dir>
set -e
export TMPDIR=/tmp
OUT=${1:?usage: bash tools/pmc_gemv.sh <output dir>}
mkdir -p "$OUT"
rm -rf "$OUT/pmc_f" "$OUT/pmc_w"
timeout -s KILL 120 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/pmc_f" -o f -- python3 bench.py --full --no-gemm --no-cpu --steps 10 --warmup 2 > "$OUT/pmc_f.log" 2>&1
timeout -s KILL 120 rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$OUT/pmc_w" -o w -- python3 bench.py --full --no-gemm --no-cpu --steps 10 --warmup 2 > "$OUT/pmc_w.log" 2>&1
F=$(find "$OUT/pmc_f" -name "*counter_collection.csv" | head -1)
W=$(find "$OUT/pmc_w" -name "*counter_collection.csv" | head -1)
python3 tools/pmc_traffic.py "$F" "$W" gemv_stream_dma_kernel "$OUT/traffic_q4_0_gemv.json" 312111360
