# pipelined step with the matcher's stream CU-masked (bench --match-cus K)
set -o pipefail
cd "$(git rev-parse --show-toplevel)"
mkdir -p ${OUT_ROOT:-out}/probe
for wl in c4 c1; do
  for k in 0 32 64 128 0 32 64 128; do
    timeout -k 10 120 python bench.py --full --workload $wl --steps 20 --warmup 3 --no-cpu-baseline --no-latency --match-cus $k > ${OUT_ROOT:-out}/probe/cum_${wl}_$k.json 2> ${OUT_ROOT:-out}/probe/cum_${wl}_$k.err || { tail -5 ${OUT_ROOT:-out}/probe/cum_${wl}_$k.err; exit 1; }
    python3 -c "import json,sys;d=json.load(open(sys.argv[1]));print(sys.argv[2], d['value'], d['ms_per_step'])" ${OUT_ROOT:-out}/probe/cum_${wl}_$k.json "$wl cus=$k"
  done
done
