#!/bin/bash
OUT=${1:?usage: tools/dev/r6_run2.sh OUTDIR}; mkdir -p $OUT
timeout 1500 python -m pytest tests -m gpu -x -q > $OUT/gputest2.log 2>&1; echo "pytest rc=$?"
tail -4 $OUT/gputest2.log
python bench.py --full --steps 20 --warmup 5 > $OUT/bench1.json 2> $OUT/bench1.err; echo "bench rc=$?"
python -c "import json;d=json.load(open('$OUT/bench1.json'));print(d['ms_per_step'],d['roofline']['frac'],d['roofline']['frac_pipeline'],d.get('steady'),d['c3_16384']['ms_per_image'],d['c3_16384']['roofline']['frac'])"
