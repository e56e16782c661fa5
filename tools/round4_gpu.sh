#!/bin/bash
# round4_gpu.sh TAG [pytest args] -- one gpurun call: the GPU test suite (timed) and the bench line.
cd "$(dirname "$0")/.."
TAG=${1:-r04a}
OUT=${OUT:-out}; mkdir -p "$OUT"
( time python -m pytest tests -m gpu -x -q -p no:cacheprovider $2 ) > $OUT/${TAG}_pytest.log 2>&1
tail -15 $OUT/${TAG}_pytest.log
python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
tail -c 1500 $OUT/${TAG}_bench.err
python tools/bench_brief.py $TAG < $OUT/${TAG}_bench.json; tail -c 2500 $OUT/${TAG}_bench.json
