#!/bin/bash
# round 6, GPU call 1: the new stage tests + whole GPU suite, a baseline bench line, the blur kernel's counters, the issue-rate ubenches
OUT=${1:?usage: tools/dev/r6_run1.sh OUTDIR}; mkdir -p $OUT
timeout 1500 python -m pytest tests -m gpu -x -q > $OUT/gputest.log 2>&1; echo "pytest rc=$?"
tail -5 $OUT/gputest.log
python bench.py --full --steps 20 --warmup 5 > $OUT/bench0.json 2> $OUT/bench0.err; echo "bench rc=$?"
python -c "import json;d=json.load(open('$OUT/bench0.json'));print(d['ms_per_step'],d['roofline']['frac'],d['roofline']['frac_pipeline'],d.get('steady'))"
bash tools/dev/pmc_blur.sh > $OUT/pmc_blur_team_kernel.txt 2>&1
./tools/ubench/valu_rate_bench > $OUT/valu_issue_rate.txt 2>&1
./tools/ubench/valu2_bench > $OUT/valu2.txt 2>&1
tail -20 $OUT/pmc_blur_team_kernel.txt
