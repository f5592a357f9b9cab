#!/bin/bash
# the committed bench records of the round (profiles/<round>/bench_*.json), on the GPU box: bash tools/bench_records.sh r03
# (full lines: kernel table, roofline, breakdown, CPU baseline; written under ${WN_OUT_DIR:-bench_out}/<round>/)
R=${1:-r03}
OUT=${WN_OUT_DIR:-bench_out}
mkdir -p $OUT/$R
python bench.py --full --steps 10 --warmup 3 > $OUT/$R/bench_cfg3_f32.json 2> $OUT/$R/bench_cfg3_f32.err
python bench.py --full --precision f16x3 --steps 10 --warmup 3 --no-cpu-baseline > $OUT/$R/bench_cfg3_f16x3.json 2> $OUT/$R/bench_cfg3_f16x3.err
python bench.py --full --config cfg2 --steps 50 --warmup 5 > $OUT/$R/bench_cfg2_bf16.json 2> $OUT/$R/bench_cfg2_bf16.err
python bench.py --full --config cfg2 --graph off --steps 50 --warmup 5 --no-cpu-baseline > $OUT/$R/bench_cfg2_bf16_eager.json 2> $OUT/$R/bench_cfg2_bf16_eager.err
WN_COL_BWD=0 python bench.py --full --config cfg2 --steps 50 --warmup 5 --no-cpu-baseline > $OUT/$R/bench_cfg2_bf16_tiled_bwd.json 2> $OUT/$R/bench_cfg2_bf16_tiled_bwd.err
WN_COL_PAIR=0 python bench.py --full --config cfg2 --steps 50 --warmup 5 --no-cpu-baseline > $OUT/$R/bench_cfg2_bf16_unpaired_bwd.json 2> $OUT/$R/bench_cfg2_bf16_unpaired_bwd.err
python bench.py --full --config cfg5 --steps 6 --warmup 2 --no-cpu-baseline > $OUT/$R/bench_cfg5_f16.json 2> $OUT/$R/bench_cfg5_f16.err
python bench.py --full --config cfg5 --precision f32 --steps 4 --warmup 1 --no-cpu-baseline > $OUT/$R/bench_cfg5_f32.json 2> $OUT/$R/bench_cfg5_f32.err
grep -h "timed" $OUT/$R/bench_*.err
