set -o pipefail
cd "$(git rev-parse --show-toplevel)"
for v in prev "" prev ""; do
  ORBX_VARIANT=$v timeout -k 10 120 python bench.py --full --workload c5 --steps 10 --warmup 2 --batch 64 --no-cpu-baseline > ${OUT_ROOT:-out}/c5_$v.json 2>${OUT_ROOT:-out}/c5_$v.err || exit $?
  python -c "import json,sys;d=json.load(open(sys.argv[1]));print('c5', sys.argv[2], d['value'], d.get('stages_ms_per_step'))" ${OUT_ROOT:-out}/c5_$v.json "v=$v"
done
