#!/bin/bash
# attention_x3's timing ablations (DI_ATTN_X3_ABLATE, launch_attention_x3: 0 = the product,
# 1 no softmax arithmetic, 2 no S^T products, 4 no O^T products -- those three in a wave's
# one-tile loop only -- 16 no second pass; wrong results, timing only) on the bench's
# encode_x3 leg, one box, alternating; attention ms per step per run.
# Usage: ABLATE="0 16 0 16" REPS=2 bash tools/ab_attn.sh
set -o pipefail
R="${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}"
OUT="$R/gpurun_out/ab_attn"
mkdir -p "$OUT"
for rep in $(seq 1 ${REPS:-2}); do
  for a in ${ABLATE:-0 16}; do
    DI_ATTN_X3_ABLATE=$a timeout -k 10 ${RUN_TIMEOUT:-240} python3 "$R/bench.py" --steps 3 --warmup 1 \
      --no-cpu --full --legs encode_x3 > "$OUT/a${a}_r${rep}.json" 2> "$OUT/a${a}_r${rep}.err" || exit $?
    python3 - "$OUT/a${a}_r${rep}.json" "$a" <<'PY'
import json, sys
for l in open(sys.argv[1]):
    if l.startswith("{"):
        d = json.loads(l)
        e = d.get("encode_fp32_faithful") or d
        k = e["kernels"]
        print(f"ablate {sys.argv[2]}: {d['value']:.1f} docs/s attention {k['attention']['ms_per_step']:.2f} ms/step", flush=True)
PY
  done
done
