#!/bin/bash
# A/B of the streaming 1x1 kernel (conv_s1.hip, TILE_S1) on the configs[2] shape (28 frames per launch x 3 streams): tools/ab_s1.sh reps [precisions]
# alternates BP_NO_S1=1 (the 64x64 plane tile as before) with the default plan on ONE box; prints frames/s of every region
reps=${1:-2}; shift
B="python bench.py --full --batch 28 --streams 3 --no-cpu-baseline --no-served-legs --no-flip-rate --no-side-runs --no-roofline --other-modes= --steps 60 --warmup 10 --repeats 3"
for rep in $(seq $reps); do
for prec in ${@:-f16r f16}; do
for off in 1 0; do
  if [ $off = 1 ]; then export BP_NO_S1=1; else unset BP_NO_S1; fi
  $B --precision $prec 2>/dev/null | python -c "
import sys, json
for l in sys.stdin:
    if l.startswith('{'):
        d = json.loads(l); print('$prec', 'pl64 ' if '$off' == '1' else 's1   ', d['value'], d.get('repeats', {}).get('fps'), 'poses', d.get('poses'))
"
done
done
done
