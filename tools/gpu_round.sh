# GPU box: full -m gpu suite, then the default bench line (N=1), each bounded
set -o pipefail
cd "$(git rev-parse --show-toplevel)"
mkdir -p ${OUT_ROOT:-out}
TAG=${1:-t}
TAG=$TAG bash tools/gpu_tests.sh || exit $?
timeout -k 10 400 python bench.py --full > ${OUT_ROOT:-out}/bench_$TAG.json 2> ${OUT_ROOT:-out}/bench_$TAG.err || exit $?
cat ${OUT_ROOT:-out}/bench_$TAG.json
