set -o pipefail
cd "$(git rev-parse --show-toplevel)"
timeout -k 10 300 python bench.py --full --steps 5 --warmup 2 --batch 64 > ${OUT_ROOT:-out}/bench1.json 2> ${OUT_ROOT:-out}/bench1.err
rc=$?; echo "bench rc=$rc" >> ${OUT_ROOT:-out}/bench1.err; [ $rc -eq 0 ] || exit $rc
export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $PWD/${OUT_ROOT:-out}/prof1 -o run -- python3 $PWD/bench.py --full --steps 5 --warmup 2 --batch 64 --no-cpu-baseline > ${OUT_ROOT:-out}/prof1.log 2>&1
echo "prof rc=$?" >> ${OUT_ROOT:-out}/prof1.log
