#!/bin/bash
# full validation of a round on the GPU box: every GPU test, smoke, the full bench line, the per-config evidence profiles; stops at the first failure
#   bash tools/gpu_round_full.sh <tag>      → $OUT/full_*.{log,json} (default results/); the profiles where tools/gpu_round5_evidence.sh writes them
tag=${1:-r5_v3}
cd "$(dirname "$0")/.."
O=${OUT:-results}; mkdir -p $O
( timeout 1800 python -X faulthandler -m pytest tests -x -q -m gpu --durations=12 2>&1 | tail -45 ) > $O/full_tests.log 2>&1 \
&& ( timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/full_smoke.log 2>&1 ) \
&& ( timeout 900 python bench.py --full > $O/full_bench.json 2> $O/full_bench.err ) \
&& ( timeout 1800 bash tools/gpu_round5_evidence.sh $tag > $O/full_profile.log 2>&1 )
tail -n 4 $O/full_tests.log; tail -n 2 $O/full_smoke.log; head -c 400 $O/full_bench.json
