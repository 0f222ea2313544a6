#!/bin/bash
# A/B of the fused step's shared face passes (profiles/face_share): a tree of
# the parent commit (built, PARENT=its root), this tree with STSP_FUSED_SHARE=0
# (every face a full face, the parent's order) and this tree's default,
# interleaved, REPS reps each, in one run.  Per rep and form: bench.py
# (defaults), bench.py 20/5 and the C96 probe (100 steps per launch).
#   PARENT=/path/to/parent OUT=bench_outputs/face_share bash tools/face_share_ab.sh
# (from the repository root; OUT: where the raw outputs and ab_summary.txt go).
# Every step runs under its own time limit and the first failure ends the run.
ROOT=$(pwd)
OUT=${OUT:-$ROOT/bench_outputs/face_share}
REPS=${REPS:-3}
FORMS=${FORMS:-"parent share0 new"}
mkdir -p $OUT
for rep in $(seq 1 $REPS); do
  for v in $FORMS; do
    cd $ROOT
    unset STSP_FUSED_SHARE
    [ $v = parent ] && cd $PARENT
    [ $v = share0 ] && export STSP_FUSED_SHARE=0
    timeout -k 10 180 python -u bench.py > $OUT/bench_${v}_$rep.json 2> $OUT/bench_${v}_$rep.err || exit $?
    timeout -k 10 180 python -u bench.py --gpus 1 --steps 20 --warmup 5 > $OUT/bench20_${v}_$rep.json 2> $OUT/bench20_${v}_$rep.err || exit $?
    timeout -k 10 120 python -u tools/fused_probe.py --N 96 --t 2 > $OUT/probe_C96_${v}_$rep.json 2> $OUT/probe_C96_${v}_$rep.err || exit $?
    python - $OUT $v $rep <<'EOF' | tee -a $OUT/ab_summary.txt
import json, sys
out, v, rep = sys.argv[1:4]
last = lambda p: json.loads(open(p).read().strip().splitlines()[-1])
a, b, c = last(f"{out}/bench_{v}_{rep}.json"), last(f"{out}/bench20_{v}_{rep}.json"), last(f"{out}/probe_C96_{v}_{rep}.json")
print(f"{v:6s} {rep} bench {a['ms_per_step'] * 1e3:.3f} us | bench 20/5 {b['ms_per_step'] * 1e3:.3f} us"
      f" | C96 probe multi20/100 {c['multi20_us_per_step']:.3f}/{c['multi100_us_per_step']:.3f}", flush=True)
EOF
  done
done
echo "== face_share_ab done"
