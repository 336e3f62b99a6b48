#!/bin/bash
# fp64-path library-kernel check + RF transform timing (one GPU call). Logs go under $OUT.
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 300 python -u -m pytest tests/test_ops_gpu.py -m gpu -k "rf_predict" -x -q --timeout 120 --timeout-method thread > $OUT/cp_pytest.log 2>&1 \
  || { echo "pytest failed"; tail -40 $OUT/cp_pytest.log; exit 1; }
tail -1 $OUT/cp_pytest.log
rm -rf $OUT/fp64
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/fp64 -o fp64 -- python3 tools/fp64_paths.py > $OUT/fp64.log 2>&1 \
  || { echo "fp64 run failed"; tail -30 $OUT/fp64.log; exit 1; }
grep -v "^W\|warn" $OUT/fp64.log | tail -8
f=$(find $OUT/fp64 -name "*kernel_stats.csv" | head -1)
python tools/fp64_paths.py --check "$f" || true
# --full: the transform pass per workload is timed only there
timeout -k 10 600 python -u bench.py --full --rows 1000000 --steps 1 --warmup 1 --algos random_forest_classifier,random_forest_regressor,pca,logistic_regression > $OUT/cp_bench.json 2> $OUT/cp_bench.err \
  || { echo "bench failed"; tail -30 $OUT/cp_bench.err; exit 1; }
python - "$OUT/cp_bench.json" <<'PY'
import json
import sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
for k, v in d["config"]["workloads"].items():
    print("  %-26s fit %.4f s  transform %s  %s" % (k, v["fit_s"], v.get("transform_s"), v.get("transform_error", "")))
PY
