# resolve-walk statistics (RS_STATS variant: per node pair rows / feasible
# rows / chunks / rounds / rescans for the first 4 units of a launch)
set -o pipefail
cd "$(git rev-parse --show-toplevel)"
mkdir -p ${OUT_ROOT:-out}/probe
for wl in c4 c1 c2 c5; do
  ORBX_VARIANT=rst timeout -k 10 120 python bench.py --full --steps 1 --warmup 0 --workload $wl --no-cpu-baseline --no-latency --serial > ${OUT_ROOT:-out}/probe/rst_$wl.out 2> ${OUT_ROOT:-out}/probe/rst_$wl.err || exit $?
  echo "== $wl"; grep "^RS unit" ${OUT_ROOT:-out}/probe/rst_$wl.out | python3 tools/rs_agg.py
done
