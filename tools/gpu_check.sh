# tests + bench (+ optional rocprof) on the GPU box; each GPU step bounded
set -o pipefail
cd "$(git rev-parse --show-toplevel)"
TAG=${1:-run}
timeout -k 10 600 python -m pytest tests -m gpu -q -p no:cacheprovider -x > ${OUT_ROOT:-out}/tests_$TAG.log 2>&1
rc=$?; echo "EXIT $rc" >> ${OUT_ROOT:-out}/tests_$TAG.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python bench.py --full --steps 10 --warmup 3 --batch 64 --no-cpu-baseline > ${OUT_ROOT:-out}/bench_$TAG.json 2> ${OUT_ROOT:-out}/bench_$TAG.err
rc=$?; echo "bench rc=$rc" >> ${OUT_ROOT:-out}/bench_$TAG.err; [ $rc -eq 0 ] || exit $rc
if [ "$2" = "prof" ]; then
  export TMPDIR=/tmp
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $PWD/${OUT_ROOT:-out}/prof_$TAG -o run -- python3 $PWD/bench.py --full --steps 5 --warmup 2 --batch 64 --no-cpu-baseline > ${OUT_ROOT:-out}/prof_$TAG.log 2>&1
  echo "prof rc=$?" >> ${OUT_ROOT:-out}/prof_$TAG.log
fi
