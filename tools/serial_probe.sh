# stage times of profiling variants in the serial loop (no pipelined-vs-serial
# equality check: variants that break the pixels on purpose); profiling only
#   VARS="name[:ENV=val] ..." BATCH=256 WL=c4 bash tools/serial_probe.sh
set -o pipefail
cd "$(git rev-parse --show-toplevel)"
mkdir -p ${OUT_ROOT:-out}/probe
for spec in ${VARS:-base}; do
  name=${spec%%:*}; envs=""
  [ "$spec" != "$name" ] && envs=${spec#*:}
  vv=""; [ "$name" != "base" ] && vv=$name
  env ORBX_VARIANT=$vv $envs timeout -k 10 120 python bench.py --full --steps ${STEPS:-10} --warmup 2 --batch ${BATCH:-64} --workload ${WL:-c4} --no-cpu-baseline --no-latency --serial > ${OUT_ROOT:-out}/probe/ser_$spec.json 2> ${OUT_ROOT:-out}/probe/ser_$spec.err || exit $?
  python -c "import json,sys;d=json.load(open(sys.argv[1]));print(sys.argv[2], d['stages_ms_per_step'])" ${OUT_ROOT:-out}/probe/ser_$spec.json "$spec"
done
