# Round-end rehearsal at HEAD: GPU tests, smoke, default bench line (driver's commands)
OUT_DIR=${OUT_DIR:-bench_out}  # where the logs and result lines go
set -o pipefail
mkdir -p $OUT_DIR
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT_DIR/final_pytest_gpu.txt 2>&1 || { tail -40 $OUT_DIR/final_pytest_gpu.txt; exit 1; }
tail -3 $OUT_DIR/final_pytest_gpu.txt
timeout -k 10 400 python -c "import __graft_entry__ as g; g.smoke()" > $OUT_DIR/final_smoke.txt 2>&1 || { tail -20 $OUT_DIR/final_smoke.txt; exit 1; }
tail -2 $OUT_DIR/final_smoke.txt
timeout -k 10 600 python bench.py --full > $OUT_DIR/final_bench.txt 2>&1 || { tail -20 $OUT_DIR/final_bench.txt; exit 1; }
tail -1 $OUT_DIR/final_bench.txt
