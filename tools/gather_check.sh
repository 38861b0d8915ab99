OUT_DIR=${OUT_DIR:-bench_out}  # where the logs and result lines go
set -u
mkdir -p $OUT_DIR
for spec in "2 cfg2" "3 cfg3"; do
  set -- $spec
  timeout -k 10 300 python bench.py --full --gpus $1 --config $2 --backend gloo --steps 4 --warmup 1 --no-cpu-baseline --no-host-path --verify-gather > $OUT_DIR/gc_gloo_$1_$2.txt 2>&1 || { tail -30 $OUT_DIR/gc_gloo_$1_$2.txt; exit 1; }
  grep "verify-gather" $OUT_DIR/gc_gloo_$1_$2.txt
done
timeout -k 10 300 python bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --no-host-path > $OUT_DIR/gc_n1.txt 2>&1 || { tail -30 $OUT_DIR/gc_n1.txt; exit 1; }
grep '^{' $OUT_DIR/gc_n1.txt | cut -c1-330
