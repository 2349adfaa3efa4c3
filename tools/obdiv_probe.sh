# k_orient_brief grid-size probe (ORBX_DEBUG_OBDIV); profiling only
set -o pipefail
cd "$(git rev-parse --show-toplevel)"
mkdir -p ${OUT_ROOT:-out}/probe
for v in ${DIVS:-1 2 4}; do
  ORBX_DEBUG_OBDIV=$v timeout -k 10 120 python bench.py --full --steps 10 --warmup 2 --batch 64 --no-cpu-baseline > ${OUT_ROOT:-out}/probe/ob$v.json 2> ${OUT_ROOT:-out}/probe/ob$v.err || exit $?
  python -c "import json;d=json.load(open('${OUT_ROOT:-out}/probe/ob$v.json'));print('div $v', d['value'], d['stages_ms_per_step'])"
done
