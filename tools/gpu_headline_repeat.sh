#!/bin/bash
# the full bench command N times on one box: how far the compact line's figures move from run to run   (results in $OUT, default results/headline_repeat)
cd "$(dirname "$0")/.."; O=${OUT:-results/headline_repeat}; mkdir -p $O
for i in $(seq 1 ${1:-3}); do
  python bench.py --gpus 1 --steps 20 --warmup 5 --full --detail-out $O/detail_$i.json 2>/dev/null | tee $O/line_$i.json | python -c "
import json,sys; t=sys.stdin.read().strip().splitlines()[-1]; j=json.loads(t); x=j['step_excludes']; c=j['cpu_baseline']
print('run $i: bytes', len(t), 'value', j['value'], 'regions', j['regions_ms_per_step'], 'lazy', x.get('lazy_flat_array'), 'host_io', x.get('host_io'), 'pipelined', j['pipelined']['value'],
      'extras', [e.get('value') for e in j['extra_configs']], 'parity', all(e['parity']['equal'] for e in j['extra_configs']) and j['parity']['equal'],
      'cpu', c['value'], c.get('legs'), c.get('host_load_1m'))"
done 2>&1 | tee $O/summary.log
