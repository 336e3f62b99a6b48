#!/bin/bash
# PMC of the IVF-PQ scan kernels at the docs/performance.md configuration (1M x 128, M = 32,
# 8-bit codes, nprobe 32): LDS bank conflicts of the data-dependent table lookups and wave
# states. Counters only, in a run of their own.
#   bash tools/pmc_ivfpq.sh [output directory, default bench_out/pmc_ivfpq]
set -o pipefail
OUT=${1:-bench_out/pmc_ivfpq}
mkdir -p "$OUT"
export TMPDIR=/tmp
P="python3 tools/ivfpq_bench.py --reps 1"
timeout -s KILL 150 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS -d "$OUT/p1" -o p1 --output-format csv -- $P > "$OUT/p1.log" 2>&1 || { tail -5 "$OUT/p1.log"; exit 1; }
for k in ivfpq_search_kernel ivfpq_candidates_kernel pq_encode_kernel ivf_search_kernel; do
  echo "== $k"
  python3 tools/pmc_summary.py $k "$OUT"
done
