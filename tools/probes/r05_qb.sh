set -o pipefail
cd "$(git rev-parse --show-toplevel)"
for wl in c4 c1 c2 c5; do
timeout -k 10 300 python bench.py --full --workload $wl --steps 20 --warmup 5 --no-cpu-baseline --no-latency > ${OUT_ROOT:-out}/qb_$wl.json 2> ${OUT_ROOT:-out}/qb_$wl.err || exit $?
python3 -c "import json,sys;d=json.load(open(sys.argv[1]));print(sys.argv[2], d['value'], d['ms_per_step'], d['serial']['value'])" ${OUT_ROOT:-out}/qb_$wl.json $wl
done
