set -o pipefail
cd "$(git rev-parse --show-toplevel)"
export TMPDIR=/tmp
OUT=$PWD/${OUT_ROOT:-out}/trace_c4p
mkdir -p $OUT
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $OUT -o run -- python3 bench.py --full --workload ${WL:-c4} --steps 10 --warmup 3 --no-cpu-baseline --no-latency > $OUT/log 2>&1 || exit $?
ls $OUT
