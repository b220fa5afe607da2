#!/bin/bash
# Counters-only passes (no tracing alongside) over the XCD-local step pipeline's walking step at n = 800, one per
# form of the dW1 pixel operand (MlpStep.xstep_pix): L2 hits / misses and fabric read requests per step.  Each pass
# is one fresh process under its own time limit; a failed pass ends the script.  Run from the repository root on the
# GPU box:   [PMC_OUT=dir] bash scripts/gpu_pmc_xstep_pix.sh [forms...]      (default: 0 1; Outputs/pmc_xstep_pix)
set -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${PMC_OUT:-"$ROOT/Outputs/pmc_xstep_pix"}
case "$OUT" in /*) ;; *) OUT="$PWD/$OUT" ;; esac  # (the passes run from /tmp)
mkdir -p "$OUT"
FORMS=${@:-0 1}
for k in $FORMS; do
  (cd /tmp && PYTHONPATH="$ROOT" timeout -k 10 150 rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum TCC_EA0_RDREQ_sum \
    -d "$OUT" -o "pix$k" --output-format csv -- python3 "$ROOT/bench/xstep_pix_run.py" --pix "$k" --steps 200 \
    > "$OUT/pix$k.log" 2>&1)
  rc=$?
  echo "pix$k rc=$rc"
  [ $rc -eq 0 ] || { tail -5 "$OUT/pix$k.log"; exit $rc; }
done
python3 "$ROOT/scripts/pmc_xstep_pix_table.py" "$OUT" --steps 200 | tee "$OUT/table.md"
