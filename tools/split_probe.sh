# pipelined headline vs --split (sub-batches of the extraction on their own streams)
#   WLS="c4 c1" SPLITS="1 2 4" bash tools/split_probe.sh
set -o pipefail
cd "$(git rev-parse --show-toplevel)"
mkdir -p ${OUT_ROOT:-out}/split
for wl in ${WLS:-c4}; do
  for sp in ${SPLITS:-1 2}; do
    timeout -k 10 200 python bench.py --full --workload $wl --split ${sp%%:*} $( [ "$sp" != "${sp%%:*}" ] && echo --match-whole ) --steps ${STEPS:-20} --warmup 3 --no-cpu-baseline --no-latency > ${OUT_ROOT:-out}/split/b_${wl}.json 2> ${OUT_ROOT:-out}/split/b_${wl}.err || exit $?
    python -c "import json,sys;d=json.load(open(sys.argv[1]));print(sys.argv[2], 'split', sys.argv[3], d['value'], d['unit'], d['ms_per_step'])" ${OUT_ROOT:-out}/split/b_${wl}.json $wl $sp
  done
done
