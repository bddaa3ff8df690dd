"""The rerank CLI's work end to end, host route against device route (reranker.ReRanker,
--score host | device): a seeded synthetic run of the size of the cross-encoder measurement
 -- 200 queries x 1000 candidates over 20 000 passages, mean 90 tokens -- on
the xlm-roberta-base shape with seeded weights, bf16x3, tokenized by the locally built
tokenizer of tests/golden/local_tokenizer.py.

The two routes alternate in one process, each on a fresh ReRanker (cold cache / empty
store) over the same model; each is warmed once; a run's time is ReRanker.run() up to a
device synchronise (the constructor's file parsing is outside).  Reports per route the
median run as candidates/s and passages/s, the device route's "ts_sort" / "ts_score" event
totals and the share of its time spent in the encode steps, and whether the run files are
byte-equal.
    python tools/rerank_ab.py [--queries 200] [--candidates 1000] [--passages 20000]
                              [--runs 3] [--out profiles/rerank_ab.json]
"""
import argparse
import hashlib
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests" / "golden"))
import bench  # noqa: E402
import local_tokenizer  # noqa: E402
from improving_learned_index_amd.encoder import DeviceEncoder, EncoderConfig  # noqa: E402
from improving_learned_index_amd.models import DeepImpact  # noqa: E402
from improving_learned_index_amd.reranker import ReRanker  # noqa: E402


def write_run(tmp, n_passages, n_queries, n_cand, mean_words, seed):
    rng = np.random.default_rng(seed)
    words = np.array(local_tokenizer.WORDS)
    lens = np.clip(rng.poisson(mean_words, n_passages), 4, 400)
    with open(tmp / "collection.tsv", "w", encoding="utf-8") as f:
        for p, n in enumerate(lens):
            f.write(f"{p}\t{' '.join(rng.choice(words, n))}\n")
    with open(tmp / "queries.tsv", "w", encoding="utf-8") as f:
        for q in range(n_queries):
            f.write(f"{q}\t{' '.join(rng.choice(words, int(rng.integers(3, 9))))}\n")
    with open(tmp / "top.tsv", "w", encoding="utf-8") as f:
        for q in range(n_queries):
            for r, p in enumerate(rng.choice(n_passages, n_cand, replace=False), start=1):
                f.write(f"{q}\t{p}\t{r}\t{n_cand - r}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=200)
    ap.add_argument("--candidates", type=int, default=1000)
    ap.add_argument("--passages", type=int, default=20000)
    ap.add_argument("--mean_words", type=int, default=88, help="+ <s> </s>: mean 90 tokens")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--precision", choices=["bf16x3", "fp32", "bf16"], default="bf16x3")
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    a = ap.parse_args()
    torch.cuda.init()
    cfg = EncoderConfig.xlmr_base()
    enc = DeviceEncoder(bench.synthetic_state_dict(cfg, seed=0), cfg, precision=a.precision)
    model = DeepImpact(enc, local_tokenizer.build_tokenizer(), 512)
    with tempfile.TemporaryDirectory() as td:
        tmp = Path(td)
        write_run(tmp, a.passages, a.queries, a.candidates, a.mean_words, seed=21)

        def run(route, i):
            out = tmp / f"run.{route}.{i}.txt"
            rr = ReRanker(None, tmp / "top.tsv", tmp / "queries.tsv", tmp / "collection.tsv",
                          out, model=model, score=route)
            assert rr.score_route == route
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rr.run()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            row = {"s": dt, "sha1": hashlib.sha1(out.read_bytes()).hexdigest(),
                   "bytes": out.stat().st_size}
            if route == "device":
                info = rr.store.info()
                row.update(encode_s=rr.encode_ms / 1e3, ts_sort_ms=rr.store.timing("ts_sort")[0],
                           ts_score_ms=rr.store.timing("ts_score")[0],
                           store_docs=info["n_docs"], store_terms=info["n_terms"],
                           store_bytes=info["device_bytes"])
                rr.store.close()
            else:
                row["store_docs"] = len(rr.cache)
            out.unlink()
            return row

        res = {"host": [], "device": []}
        run("device", "warm")
        run("host", "warm")
        for i in range(a.runs):
            res["host"].append(run("host", i))
            res["device"].append(run("device", i))

    n_c = a.queries * a.candidates

    def summary(rows):
        med = statistics.median(r["s"] for r in rows)
        return {"run_s": [round(r["s"], 4) for r in rows], "median_run_s": med,
                "candidates_per_s": n_c / med, "passages_per_s": rows[0]["store_docs"] / med,
                "passages_encoded": rows[0]["store_docs"]}

    host, dev = summary(res["host"]), summary(res["device"])
    d = res["device"]
    dev.update(encode_s=statistics.median(r["encode_s"] for r in d),
               encode_share=statistics.median(r["encode_s"] / r["s"] for r in d),
               ts_sort_ms=statistics.median(r["ts_sort_ms"] for r in d),
               ts_score_ms=statistics.median(r["ts_score_ms"] for r in d),
               store_terms=d[0]["store_terms"], store_bytes=d[0]["store_bytes"])
    out = {"tool": "rerank_ab", "precision": a.precision, "queries": a.queries,
           "candidates": a.candidates, "passages": a.passages, "runs": a.runs,
           "host_route": host, "device_route": dev,
           "device_over_host": host["median_run_s"] / dev["median_run_s"],
           "bytes_equal": len({r["sha1"] for r in res["host"] + res["device"]}) == 1,
           "run_file_bytes": d[0]["bytes"]}
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
