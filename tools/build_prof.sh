# Developer diagnostic: per-kernel times of the bench loop.  Usage on the GPU box: bash tools/build_prof.sh [tag]   (results in $OUT, default results/)
R=$(cd "$(dirname "$0")/.." && pwd); tag=${1:-cur}; P=${OUT:-$R/results}/prof_$tag; mkdir -p $P; cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $P -o out -- python $R/bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --pipeline-streams 0 > $P/bench.json 2> $P/bench.err
db=$(ls $P/*.db $P/*/*.db 2>/dev/null | head -1)
python $R/tools/prof_summary.py $db $P/kernel_stats.md "$tag" | head -30
cat $P/bench.json | python -c "import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d['value'], d['ms_per_step'], d['phases_ms'])"
