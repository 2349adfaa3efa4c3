# round-end evidence on the GPU box: profiles (trace + traffic + SQ), then the
# default bench line (with the CPU baseline) using the fresh traffic summary
set -o pipefail
cd "$(git rev-parse --show-toplevel)"
TAG=${1:?tag}
bash tools/gpu_prof.sh $TAG || exit $?
timeout -k 10 600 python bench.py --full --traffic ${OUT_ROOT:-out}/prof_$TAG/traffic.json > ${OUT_ROOT:-out}/bench_$TAG.json 2> ${OUT_ROOT:-out}/bench_$TAG.err || exit $?
