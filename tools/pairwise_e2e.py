"""The pairwise index step end to end, host order against device order: the bench's encode
batch (bench.synthetic_docs_tokens: the same documents, lengths and kept terms;
xlm-roberta-base shape, synthetic weights plus a pair head) through Indexer's pool path --
the packed chunks a tokenizer pool would send (here: cut from the synthetic batch, terms
spelled "▁t<k>"), merged into device batches, DeepPairwiseImpact.encode_packed_impacts
on the main thread, formatting and the file write on the writer thread.

The two paths alternate in one process: DI_PAIRWISE_HOST_ORDER=1 (every pair score to the
host, pairwise_entries, Python-built names, di_format_impact_lines) and the default
(di_encode_pairwise_entries, di_format_entry_lines).  Reports docs/s of each (median
step), their ratio, whether the written bytes are equal, per path the main thread's time
in encode_packed_impacts and the writer's time in the formatting jobs, and from a further
DI_F_TIMING call the pair_count / pair_order / pair_merge times beside pair_attn's.
    python tools/pairwise_e2e.py [--docs 8192] [--steps 3] [--precision bf16x3]
                                 [--pair_bias 0.0]
"""
import argparse
import hashlib
import io
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402
from improving_learned_index_amd.encoder import DeviceEncoder, EncoderConfig  # noqa: E402
from improving_learned_index_amd.indexer import Indexer  # noqa: E402
from improving_learned_index_amd.models import DeepPairwiseImpact  # noqa: E402

CHUNK = 512  # documents per tokenizer-worker chunk (16 workers on an 8192-document batch)


def chunks(ids, cu, tt, ct, vocab_terms=50000):
    """The batch as the packed blobs of TokenizerPool.imap."""
    out = []
    rng = np.random.default_rng(7)
    for d0 in range(0, len(cu) - 1, CHUNK):
        d1 = min(len(cu) - 1, d0 + CHUNK)
        t0, t1 = int(ct[d0]), int(ct[d1])
        # distinct names inside a document (a map's keys): a random base plus the rank
        names = [f"▁t{(b + r) % vocab_terms}".encode()
                 for d in range(d0, d1)
                 for b in [int(rng.integers(0, vocab_terms))]
                 for r in range(int(ct[d + 1] - ct[d]))]
        off = np.zeros(len(names) + 1, np.int64)
        off[1:] = np.cumsum([len(b) for b in names])
        out.append((ids[cu[d0]:cu[d1]].copy(), (cu[d0:d1 + 1] - cu[d0]).astype(np.int32),
                    b"".join(names), off, tt[t0:t1].copy(), (ct[d0:d1 + 1] - t0).astype(np.int32)))
    return out


class Pool:
    """Stands in for TokenizerPool: the chunks are ready."""

    def __init__(self, parts, n=16):
        self.parts, self.n = parts, n

    def imap(self, _chunks):
        return iter(self.parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--max_len", type=int, default=300)
    ap.add_argument("--precision", choices=["bf16x3", "fp32"], default="bf16x3")
    ap.add_argument("--pair_bias", type=float, default=0.0,
                    help="bias of the pair head: the larger, the more pairs survive the "
                         "round-to-0.000 filter (1.0 keeps every pair)")
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    a = ap.parse_args()
    torch.cuda.init()
    cfg = EncoderConfig.xlmr_base()
    cfg.activation = "relu"
    sd = bench.synthetic_state_dict(cfg, seed=0)
    H = cfg.hidden
    w = 0.02 * np.random.default_rng(5).standard_normal(2 * H + 1).astype(np.float32)
    w[0] = 4.0
    sd["pairwise_impact_score_encoder.0.weight"] = torch.from_numpy(w.reshape(1, -1))
    sd["pairwise_impact_score_encoder.0.bias"] = torch.full((1,), a.pair_bias)
    enc = DeviceEncoder(sd, cfg, precision=a.precision)
    ids, cu, lens, tt, ct = bench.synthetic_docs_tokens(a.docs, cfg.vocab_size, seed=100,
                                                        max_len=a.max_len)
    T = np.diff(ct.astype(np.int64))
    model = DeepPairwiseImpact(enc, None, a.max_len)
    parts = chunks(ids, cu, tt, ct)
    ix = Indexer(model, pool=Pool(parts))
    stage = {}
    inner = model.encode_packed_impacts

    def timed_encode(packed):
        t0 = time.perf_counter()
        job = inner(packed)
        stage["main"] = stage.get("main", 0.0) + time.perf_counter() - t0

        def timed_job():
            t1 = time.perf_counter()
            text = job()
            stage["writer"] = stage.get("writer", 0.0) + time.perf_counter() - t1
            return text

        return timed_job

    model.encode_packed_impacts = timed_encode

    def step(host):
        if host:
            os.environ["DI_PAIRWISE_HOST_ORDER"] = "1"
        else:
            os.environ.pop("DI_PAIRWISE_HOST_ORDER", None)
        stage.clear()
        f = io.StringIO()
        batch = [None] * a.docs
        t0 = time.perf_counter()
        ix.finish((batch, ix.pool.imap(None)), f, wait=False)
        t_main = time.perf_counter() - t0
        ix.drain()
        dt = time.perf_counter() - t0
        return dt, t_main, dict(stage), hashlib.sha1(f.getvalue().encode()).hexdigest(), \
            len(f.getvalue())

    res = {"host": [], "device": []}
    step(False)  # warm-up: workspace growth, first launches
    for _ in range(a.steps):
        res["host"].append(step(True))
        res["device"].append(step(False))
    os.environ.pop("DI_PAIRWISE_HOST_ORDER", None)
    # kernel times of one device batch (DEVICE_DOCS documents, as the indexer cuts them)
    n = min(a.docs, 4096)
    for k in ("pair_attn",):
        enc.timing(k, reset=True)
    cu_out, first, _, _ = enc.encode_pairwise_entries(ids[:cu[n]], cu[:n + 1], tt[:ct[n]],
                                                      ct[:n + 1], round3=True, timing=True)
    kern = {k: enc.timing(k)[0] for k in ("pair_prep", "pair_attn", "pair_score", "pair_count",
                                          "pair_order", "pair_merge")}

    def summary(rows):
        med = statistics.median(r[0] for r in rows)
        return {"step_s": [round(r[0], 4) for r in rows], "median_step_s": med,
                "docs_per_s": a.docs / med,
                "main_thread_until_encoded_s": statistics.median(r[1] for r in rows),
                "main_thread_in_encode_packed_impacts_s":
                    statistics.median(r[2]["main"] for r in rows),
                "writer_thread_in_format_jobs_s": statistics.median(r[2]["writer"] for r in rows)}

    host, dev = summary(res["host"]), summary(res["device"])
    out = {"tool": "pairwise_e2e", "precision": a.precision, "docs": a.docs,
           "pair_bias": a.pair_bias,
           "tokens": int(cu[-1]), "terms": int(ct[-1]), "pairs": int((T * (T - 1) // 2).sum()),
           "entries_of_first_device_batch": int(cu_out[-1]), "chunk_docs": CHUNK,
           "host_order": host, "device_order": dev,
           "device_over_host_docs_per_s": dev["docs_per_s"] / host["docs_per_s"],
           "bytes_equal": len({r[3] for r in res["host"] + res["device"]}) == 1,
           "text_bytes": res["device"][0][4],
           "timer_ms_first_device_batch": kern, "timer_batch_docs": n}
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
