#!/bin/bash
# One-pass Consistency A/B on cfg4: VARIANTS (env assignments, ';'-separated per variant), ROUNDS passes
OUT_DIR=${OUT_DIR:-bench_out}  # where the logs and result lines go
set -u
mkdir -p $OUT_DIR
out=${OUT:-$OUT_DIR/lr_ab.jsonl}
IFS=';' read -ra VS <<< "${VARIANTS:-BICOS_LR_ONE_PASS=1;BICOS_LR_ONE_PASS=0}"
for r in $(seq ${ROUNDS:-2}); do
  for v in "${VS[@]}"; do
    env $v timeout -k 10 240 python bench.py --full --config ${CFG:-cfg4} --steps 100 --warmup 5 --no-cpu-baseline --no-host-path > $OUT_DIR/lr.txt 2> $OUT_DIR/lr.err
    rc=$?; if [ $rc -ne 0 ]; then echo "STOP rc=$rc"; tail -5 $OUT_DIR/lr.err; exit $rc; fi
    python - "$v" $r $OUT_DIR/lr.txt <<'PY' | tee -a $out
import json,sys
j=json.loads([l for l in open(sys.argv[3]) if l.startswith("{")][-1])
r=j["roofline"]
print(json.dumps({"variant":sys.argv[1],"round":int(sys.argv[2]),"config":j["config"]["workload"].split(":")[0],"value":j["value"],"ms_per_step":j["ms_per_step"],
 "search_ms":r["ms_per_launch"],"frac":r["frac"],"bound":r["bound"],"plan":r.get("plan"),"agree_ms":r["hbm"]["agree_ms"],"stage_ms":r.get("stage_after_transform_ms")}))
PY
  done
done
echo done
