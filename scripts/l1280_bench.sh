# configs[4]: the l-scale 701 model at 1280^2 bs 16 on one GPU, bf16 and with the fp8 forward convs
# usage: bash scripts/l1280_bench.sh <output dir>
set -o pipefail
OUT=${1:?usage: bash scripts/l1280_bench.sh <output dir>}; mkdir -p $OUT
timeout -k 10 600 python -u bench.py --full --scale l --img 1280 --bs 16 --steps 10 --warmup 3 --roofline-steps 1 --stage-check 0 > $OUT/bench.log 2>&1 || { tail -20 $OUT/bench.log; exit 1; }
grep '^{' $OUT/bench.log | tail -1 > $OUT/bench.json
timeout -k 10 600 python -u bench.py --scale l --img 1280 --bs 16 --steps 10 --warmup 3 --roofline-steps 0 --stage-check 0 --conv-fp8 > $OUT/bench_fp8.log 2>&1 || { tail -20 $OUT/bench_fp8.log; exit 1; }
grep '^{' $OUT/bench_fp8.log | tail -1 > $OUT/bench_fp8.json
python -c "
import json
for f in ('bench', 'bench_fp8'):
    d = json.load(open('$OUT/%s.json' % f))
    r = d.get('roofline') or {}
    print(f, d['ms_per_step'], d['value'], d['dtype'], (r.get('network') or {}), d['peak_hbm_gib'])
"
