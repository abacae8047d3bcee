#!/bin/bash
# Round evidence, part 2 (ROUND, default r03): standalone BA (C3, C5), line front end, FrameOptimization /
# PnP, the BASELINE C1 plumbing run (100 stereo pairs, SP/SG/lines vs the CPU restatement) and the
# 100-keyframe map-side sequence -> $OUT/${ROUND}_*.  Each step has its own time limit.
set -o pipefail
ROUND=${ROUND:-r06}
OUT=${OUT:-round_out}
mkdir -p $OUT
{ timeout -k 10 120 python -u tools/bench_ba.py --iters 50 && timeout -k 10 120 python -u tools/bench_ba.py --iters 10 --poses 30 --points 10000 --lines 0; } > $OUT/${ROUND}_bench_ba.txt || { echo "ba bench failed"; exit 1; }
cat $OUT/${ROUND}_bench_ba.txt
timeout -k 10 200 python -u tools/bench_lines.py > $OUT/${ROUND}_bench_lines.json || { echo "line bench failed"; exit 1; }
cat $OUT/${ROUND}_bench_lines.json
timeout -k 10 200 python -u tools/bench_frame.py > $OUT/${ROUND}_bench_frame.json 2> $OUT/bench_frame.err || { echo "frame bench failed"; tail -5 $OUT/bench_frame.err; exit 1; }
cat $OUT/${ROUND}_bench_frame.json
timeout -k 10 400 python -u tools/run_c1_plumbing.py --pairs 100 --out $OUT/${ROUND}_c1_pairs.jsonl > $OUT/${ROUND}_c1_plumbing.json 2> $OUT/c1.err || { echo "c1 failed"; tail -5 $OUT/c1.err; exit 1; }
cat $OUT/${ROUND}_c1_plumbing.json
timeout -k 10 500 python -u tools/run_sequence.py --out $OUT/${ROUND}_sequence > $OUT/${ROUND}_sequence100.json 2> $OUT/seq.err || { echo "sequence failed"; tail -5 $OUT/seq.err; exit 1; }
cat $OUT/${ROUND}_sequence100.json
timeout -k 10 500 python -u tools/run_sequence.py --analytic-line-jacobian --out $OUT/${ROUND}_sequence_analytic > $OUT/${ROUND}_sequence100_analytic.json 2> $OUT/seqa.err || { echo "sequence (analytic) failed"; tail -5 $OUT/seqa.err; exit 1; }
cat $OUT/${ROUND}_sequence100_analytic.json
timeout -k 10 300 python -u bench.py --full --workload c4 --steps 100 --warmup 5 --no-cpu-baseline --single-precision > $OUT/${ROUND}_bench_c4.json 2> $OUT/c4.err || { echo "c4 bench failed"; tail -5 $OUT/c4.err; exit 1; }
python3 -c "import json,sys; d=json.load(open(sys.argv[1])); print('c4', d['value'], d['ms_per_step'])" $OUT/${ROUND}_bench_c4.json
timeout -k 10 300 python -u bench.py --full --workload c5 --steps 20 --warmup 3 --no-cpu-baseline --single-precision > $OUT/${ROUND}_bench_c5.json 2> $OUT/c5.err || { echo "c5 bench failed"; tail -5 $OUT/c5.err; exit 1; }
python3 -c "import json,sys; d=json.load(open(sys.argv[1])); print('c5', d['value'], d['ms_per_step'], {k: d['stages_ms_per_step'].get(k) for k in ('sg:sinkhorn', 'sg:gnn x18', 'ba:wall')})" $OUT/${ROUND}_bench_c5.json
