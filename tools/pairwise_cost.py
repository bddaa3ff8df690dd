"""What di_encode_pairwise costs next to di_encode: alternated steps of both calls, in one
process, on the bench's encode batch (bench.synthetic_docs_tokens: the same documents,
lengths and kept terms; xlm-roberta-base shape, synthetic weights plus a pair head).

Reports the median step time of each call (device pointers, one stream, a synchronise
per step), their ratio, the pair_attn / pair_score / pair_prep timer totals per step from
a further DI_F_TIMING step, the algorithmic f32 products of pair_attn (2 * 64 * T * n per
document, layer and head, for T kept terms and n tokens) and the fraction of the f32
MFMA peak they reach in pair_attn's time.
    python tools/pairwise_cost.py [--docs 8192] [--steps 5] [--precision bf16x3]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402
from improving_learned_index_amd import _lib  # noqa: E402
from improving_learned_index_amd.encoder import DeviceEncoder, EncoderConfig  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max_len", type=int, default=300)
    ap.add_argument("--precision", choices=["bf16x3", "fp32"], default="bf16x3")
    a = ap.parse_args()
    torch.cuda.init()
    cfg = EncoderConfig.xlmr_base()
    cfg.activation = "relu"
    sd = bench.synthetic_state_dict(cfg, seed=0)
    H = cfg.hidden
    w = 0.02 * np.random.default_rng(5).standard_normal(2 * H + 1).astype(np.float32)
    w[0] = 4.0
    sd["pairwise_impact_score_encoder.0.weight"] = torch.from_numpy(w.reshape(1, -1))
    sd["pairwise_impact_score_encoder.0.bias"] = torch.zeros(1)
    enc = DeviceEncoder(sd, cfg, precision=a.precision)
    ids, cu, lens, tt, ct = bench.synthetic_docs_tokens(a.docs, cfg.vocab_size, seed=100,
                                                        max_len=a.max_len)
    T = np.diff(ct.astype(np.int64))
    cp = np.zeros(a.docs + 1, np.int64)
    cp[1:] = np.cumsum(T * (T - 1) // 2)
    n_tok, n_terms, n_pairs, max_len = int(cu[-1]), int(ct[-1]), int(cp[-1]), int(lens.max())
    enc.set_stream(torch.cuda.current_stream().cuda_stream)
    d = {k: torch.from_numpy(v).cuda() for k, v in
         dict(ids=ids, cu=cu, tt=tt, ct=ct, cp=cp).items()}
    single = torch.empty(max(1, n_terms), dtype=torch.float32, device="cuda")
    pair = torch.empty(max(1, n_pairs), dtype=torch.float32, device="cuda")
    enc.reserve(n_tok, a.docs, n_terms)
    base = _lib.DI_F_DEVICE_PTRS | _lib.DI_F_ASYNC | 0x10  # DI_F_ROUND3

    def plain(flags=base):
        enc.encode_device(d["ids"], d["cu"], a.docs, n_tok, max_len, d["tt"], d["ct"], n_terms,
                          single, flags)

    def pairwise(flags=base):
        enc.encode_pairwise_device(d["ids"], d["cu"], a.docs, n_tok, max_len, d["tt"], d["ct"],
                                   n_terms, d["cp"], n_pairs, single, pair, None, flags)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for _ in range(a.warmup):
        plain()
        pairwise()
    t_plain, t_pair = [], []
    for _ in range(a.steps):
        t_plain.append(timed(plain))
        t_pair.append(timed(pairwise))
    enc.sync()
    enc.timing("pair_attn", reset=True)
    pairwise(base | _lib.DI_F_TIMING)
    torch.cuda.synchronize()
    enc.sync()
    kern = {k: enc.timing(k)[0] for k in ("pair_prep", "pair_attn", "pair_score", "attention",
                                          "gemm_qkv")}
    mp, mw = statistics.median(t_plain), statistics.median(t_pair)
    L, nh = cfg.layers, cfg.heads
    flop = float(L * nh * 2 * 64 * (T * lens.astype(np.int64)).sum())
    attn_s = kern["pair_attn"] / 1000.0
    print(json.dumps({
        "tool": "pairwise_cost", "precision": a.precision, "docs": a.docs, "tokens": n_tok,
        "terms": n_terms, "pairs": n_pairs, "max_len": max_len, "steps": a.steps,
        "plain_step_ms": [round(x * 1e3, 2) for x in t_plain],
        "pairwise_step_ms": [round(x * 1e3, 2) for x in t_pair],
        "plain_median_ms": mp * 1e3, "pairwise_median_ms": mw * 1e3, "ratio": mw / mp,
        "timer_ms_per_step": kern, "pair_attn_tflop": flop / 1e12,
        "pair_attn_tflops": flop / attn_s / 1e12 if attn_s > 0 else None,
        "pair_attn_fraction_of_f32_mfma_peak":
            flop / attn_s / 1e12 / bench.MFMA_F32_PEAK_TFLOPS if attn_s > 0 else None}))


if __name__ == "__main__":
    main()
