#!/bin/bash
# Run on an MI355X: the whole GPU test-suite, then the bench line with every leg (--full).
cd "$(dirname "$0")/.." && REPO=$PWD
OUT=$REPO/gpurun_out/full_check; mkdir -p $OUT
timeout 2400 python -m pytest tests -x -q -m gpu 2>&1 | tail -15 > $OUT/pytest.txt
cat $OUT/pytest.txt
timeout 1500 python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err
tail -1 $OUT/bench_default.json | cut -c1-6000
tail -5 $OUT/bench_default.err
