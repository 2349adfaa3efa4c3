# bench throughput vs frames per step (1 GPU)
set -o pipefail
cd "$(git rev-parse --show-toplevel)"
mkdir -p ${OUT_ROOT:-out}/sweep
for b in ${BATCHES:-32 64 128 256}; do
  timeout -k 10 240 python bench.py --full --steps 10 --warmup 2 --batch $b --no-cpu-baseline > ${OUT_ROOT:-out}/sweep/b$b.json 2> ${OUT_ROOT:-out}/sweep/b$b.err || exit $?
done
