# k_pyramid time vs last-level tile size (ORBX_DEBUG_PYR_TILE); profiling only
set -o pipefail
cd "$(git rev-parse --show-toplevel)"
mkdir -p ${OUT_ROOT:-out}/pyr
for k in ${TILES:-0 1 2 3 4}; do
  ORBX_DEBUG_PYR_TILE=$k timeout -k 10 120 python bench.py --full --steps 10 --warmup 2 --batch 64 --no-cpu-baseline > ${OUT_ROOT:-out}/pyr/t$k.json 2> ${OUT_ROOT:-out}/pyr/t$k.err || exit $?
done
