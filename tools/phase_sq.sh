# SQ instruction mix / wait split of k_fast_strips per kernel phase
# (ORBX_DEBUG_STOP cut-offs of a profiling variant; profiling only):
#   VAR=new PHASES="1 5 2 3 0" WL=c4 bash tools/phase_sq.sh TAG
# -> ${OUT_ROOT:-out}/phsq_TAG/v<phase>/run_counter_collection.csv; summarise with
#    python3 tools/phase_sq_summary.py ${OUT_ROOT:-out}/phsq_TAG
# Cut-offs 2 / 3 / 4 since the per-strip post-pass (round 7):
#   2     every strip stops after the barrier that ends pass 1 (as before);
#   3, 4  a dense strip (> 64 corners, or more than its list holds) stops after
#         the NMS into the row masks, as before; a sparse strip (1..64 corners)
#         stops once wave 0 has its lanes' two kept flags (its NMS: no ranks, no
#         keys, no counts written); an empty strip has no NMS and no output
#         phase: it writes its cells' zero counts and ends, at any cut-off > 2.
#   So "3 - 2" is the NMS of dense strips + the kept flags of sparse ones + the
#   zero counts of empty ones, and "0 - 3" the dense strips' mask output + the
#   sparse strips' rank loop, key and count stores.
set -o pipefail
cd "$(git rev-parse --show-toplevel)"
TAG=${1:-run}
export TMPDIR=/tmp
OUT=$PWD/${OUT_ROOT:-out}/phsq_$TAG
mkdir -p $OUT
ARGS="--steps 2 --warmup 1 --workload ${WL:-c4} --batch ${BATCH:-0} --no-cpu-baseline --no-latency --serial"
for v in ${PHASES:-1 5 2 3 0}; do
  ORBX_VARIANT=${VAR:-new} ORBX_DEBUG_STOP=$v timeout -s KILL 120 rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS --output-format csv -d $OUT/v$v -o run -- python3 $PWD/bench.py --full $ARGS > $OUT/v$v.log 2>&1 || exit $?
  echo "phase $v done"
done
