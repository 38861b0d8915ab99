OUT_DIR=${OUT_DIR:-bench_out}  # where the logs and result lines go
set -o pipefail
mkdir -p $OUT_DIR
for c in cfg2 cfg1 cfg3 cfg4 cfg5 readme; do
  timeout -k 10 400 python bench.py --full --config $c --no-host-path > $OUT_DIR/allcfg_$c.txt 2>&1 || { tail -5 $OUT_DIR/allcfg_$c.txt; exit 1; }
  tail -1 $OUT_DIR/allcfg_$c.txt | cut -c1-200
done
