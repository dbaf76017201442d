# configs[4] on one GPU: l-scale 1280^2 bs16 train step, bf16 and with the fp8 forward-conv engine
# usage: bash scripts/l1280_fp8.sh <output dir>
set -o pipefail
OUT=${1:?usage: bash scripts/l1280_fp8.sh <output dir>}; mkdir -p $OUT
timeout -k 10 500 python -u bench.py --full --scale l --img 1280 --bs 16 --steps 5 --warmup 2 --roofline-steps 1 > $OUT/bf16.log 2>&1 || { tail -5 $OUT/bf16.log; exit 1; }
timeout -k 10 500 python -u bench.py --full --scale l --img 1280 --bs 16 --steps 5 --warmup 2 --roofline-steps 1 --conv-fp8 > $OUT/fp8.log 2>&1 || { tail -5 $OUT/fp8.log; exit 1; }
for f in bf16 fp8; do grep -o '"value": [0-9.]*, "unit": "images/s", "n_gpus": 1, "steps": 5, "warmup": 2, "ms_per_step": [0-9.]*' $OUT/$f.log; done
