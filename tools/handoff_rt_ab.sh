#!/bin/bash
# A/B of the fused step's hand-off round trips (profiles/handoff_rt): library
# variants interleaved, three reps each, in one run.  hrt0 = the hand-off as
# it was (tail cells on ring-owning threads, xg_wait, inner faces on every
# wave), hrt1 = tail cells moved, hrt12 = + fused_wait, "" = production
# (+ ring-first polls).  Per rep and variant: the in-kernel probe at C96 (with
# stamps: per-wave ring arrival) and at C36 B = 6, bench.py 20/5 and default.
#   python -m stsphere.ops.build --variant hrt0   (etc., before the run)
#   OUT=bench_outputs/handoff_rt VARIANTS="hrt0 hrt1 hrt12 prod" bash tools/handoff_rt_ab.sh
# (from the repository root; OUT: where the raw outputs and ab_summary.txt go)
ROOT=$(pwd)
OUT=${OUT:-$ROOT/bench_outputs/handoff_rt}
VARIANTS=${VARIANTS:-"hrt0 prod"}
mkdir -p $OUT
cd $ROOT
for rep in 1 2 3; do
  for v in $VARIANTS; do
    export STSP_VARIANT=$v
    [ $v = prod ] && export STSP_VARIANT=
    timeout -k 10 120 python -u tools/fused_probe.py --N 96 --t 2 --stamps > $OUT/probe_C96_${v}_$rep.json 2> $OUT/probe_C96_${v}_$rep.err || exit $?
    timeout -k 10 120 python -u tools/fused_probe.py --N 36 --t 1 --B 6 > $OUT/probe_C36B6_${v}_$rep.json 2> $OUT/probe_C36B6_${v}_$rep.err || exit $?
    timeout -k 10 180 python -u bench.py --gpus 1 --steps 20 --warmup 5 > $OUT/bench20_${v}_$rep.json 2> $OUT/bench20_${v}_$rep.err || exit $?
    timeout -k 10 180 python -u bench.py > $OUT/bench_${v}_$rep.json 2> $OUT/bench_${v}_$rep.err || exit $?
    python -u tools/handoff_rt_row.py $OUT $v $rep | tee -a $OUT/ab_summary.txt
  done
done
echo "== handoff_rt_ab done"
