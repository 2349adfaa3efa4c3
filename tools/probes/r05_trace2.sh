# kernel trace of the driver's c4 command shape (20 steps, warmup 5): step
# spacing inside the pipelined window, fill and drain
set -o pipefail
cd "$(git rev-parse --show-toplevel)"
export TMPDIR=/tmp
OUT=$PWD/${OUT_ROOT:-out}/trace_c4w
mkdir -p $OUT
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $OUT -o run -- python3 bench.py --full --workload c4 --steps 20 --warmup 5 --no-cpu-baseline --no-latency > $OUT/log 2>&1 || exit $?
ls $OUT
