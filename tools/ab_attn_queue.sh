#!/bin/bash
# A/B of attention_x3's unit order (DI_ATTN_X3_QUEUE, launch_attention_x3: 0 = the documents
# as they come, 1 = longest first in one launch per layer, 2 = longest first and the two
# forms) on the plain bench run, one box, alternating; per run docs/s, attention ms per
# step and out_sha1.  "lib:PATH" as a variant runs another build of the library (a parent
# commit's) with the knob unset.
# OUT: where the runs' outputs go (default: a fresh temporary directory).
# Usage: VARIANTS="lib:parent/libdeepimpact_hip.so 0 1 2" REPS=3 bash tools/ab_attn_queue.sh
set -o pipefail
R="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${OUT:-$(mktemp -d)}"  # the runs' JSON lines and stderr
mkdir -p "$OUT"
for rep in $(seq 1 ${REPS:-3}); do
  i=0
  for v in ${VARIANTS:-0 1 2}; do
    i=$((i + 1))
    f="$OUT/v${i}_r${rep}"
    if [ "${v#lib:}" != "$v" ]; then
      env -u DI_ATTN_X3_QUEUE DEEPIMPACT_HIP_LIB="${v#lib:}" timeout -k 10 ${RUN_TIMEOUT:-240} \
        python3 "$R/bench.py" --steps ${STEPS:-20} --warmup ${WARMUP:-5} > "$f.json" 2> "$f.err" || exit $?
    else
      DI_ATTN_X3_QUEUE=$v timeout -k 10 ${RUN_TIMEOUT:-240} \
        python3 "$R/bench.py" --steps ${STEPS:-20} --warmup ${WARMUP:-5} > "$f.json" 2> "$f.err" || exit $?
    fi
    python3 - "$f.json" "$v" <<'PY'
import json, sys
for l in open(sys.argv[1]):
    if l.startswith("{"):
        d = json.loads(l)
        e = d["encode_fp32_faithful"]
        k = e["kernels"]
        print(f"DI_ATTN_X3_QUEUE={sys.argv[2]}  {d['value']:.1f} docs/s " +
              " ".join(f"{n}={k[n]['ms_per_step']:.2f}" for n in
                       ("gemm_qkv", "attention", "gemm_o", "gemm_ffn1", "gemm_ffn2")) +
              f" sha1={e['out_sha1'][:10]}", flush=True)
PY
  done
done
