set -o pipefail
cd "$(git rev-parse --show-toplevel)"
TAG=r05g1 bash tools/gpu_tests.sh tests || { tail -40 ${OUT_ROOT:-out}/gtests_r05g1.log; exit 1; }
tail -2 ${OUT_ROOT:-out}/gtests_r05g1.log
timeout -k 10 300 python bench.py --full --workload c4 > ${OUT_ROOT:-out}/r05g1_bench_c4.json 2> ${OUT_ROOT:-out}/r05g1_bench_c4.err || exit $?
head -c 600 ${OUT_ROOT:-out}/r05g1_bench_c4.json
