# last check of the tree the driver runs: full GPU suite, smoke, and the
# driver's bench command (1 GPU, 20 steps, 5 warm-up)
set -o pipefail
cd "$(git rev-parse --show-toplevel)"
TAG=r05last bash tools/gpu_tests.sh tests || { tail -30 ${OUT_ROOT:-out}/gtests_r05last.log; exit 1; }
tail -1 ${OUT_ROOT:-out}/gtests_r05last.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" || exit 1
mkdir -p ${OUT_ROOT:-out}/last
timeout -k 10 900 python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > ${OUT_ROOT:-out}/last/bench.json 2> ${OUT_ROOT:-out}/last/bench.err || exit 1
python3 -c "import json;L=open('${OUT_ROOT:-out}/last/bench.json').read().splitlines();assert len(L)==1;d=json.loads(L[0]);print(d['value'], d['ms_per_step'], d['roofline']['frac'], d['cpu_baseline']['value'], d['latency']['search_by_bow_2000x2000']['p50_us'])"
