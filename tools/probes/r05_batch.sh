set -o pipefail
cd "$(git rev-parse --show-toplevel)"
for b in 256 384 512 256 512; do
timeout -k 10 300 python bench.py --full --workload c4 --batch $b --steps 20 --warmup 5 --no-cpu-baseline --no-latency > ${OUT_ROOT:-out}/bt.json 2> ${OUT_ROOT:-out}/bt.err || { tail -5 ${OUT_ROOT:-out}/bt.err; exit 1; }
python3 -c "import json,sys;d=json.load(open(sys.argv[1]));print(sys.argv[2], d['value'], d['ms_per_step'], d['serial']['value'])" ${OUT_ROOT:-out}/bt.json $b
done
