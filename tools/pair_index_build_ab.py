"""From a collection to a searchable quantized index for the pairwise model, text route
against direct route: the seeded synthetic passages of tools/index_build_ab.py (mean 90
tokens, the words of tests/golden/local_tokenizer.py) on the xlm-roberta-base shape with
seeded weights and the pair head of tools/pairwise_e2e.py, bf16x3.

  text route    Indexer.index (DeepPairwiseImpact: every 't1|t2' entry into the impact
                TSV), quantize_file, create_index, InvertedIndex(path)
  direct route  Indexer.build_index(index_path=...): single and pair scores stay on the
                device, di_index_builder_append_pairwise keeps the pairs that do not round
                to zero, di_index_builder_quantize numbers the distinct pair keys

The two routes alternate in one process over the same model and the same batches, each
warmed once; a run ends with a device synchronise.  Reports per route the runs, their
median, fastest and spread, the direct route's DI_F_TIMING regions, the TSV's bytes and
the postings per passage, the count of distinct pair terms, whether the three files are
byte-equal, whether the queries rank equally, and the verdict of DESIGN.md §3's rule: the
direct route counts as faster only if its median is below the text route's fastest run.
    python tools/pair_index_build_ab.py [--passages 2000] [--queries 50] [--runs 3]
                                        [--out profiles/pair_index_build_ab.json]
"""
import argparse
import json
import shutil
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
from improving_learned_index_amd.indexer import Indexer  # noqa: E402
from improving_learned_index_amd.inverted_index import InvertedIndex, create_index  # noqa: E402
from improving_learned_index_amd.models import DeepPairwiseImpact  # noqa: E402
from improving_learned_index_amd.quantize import quantize_file  # noqa: E402
from sparse_build_ab import make_corpus  # noqa: E402


class Timed(DeepPairwiseImpact):
    """DeepPairwiseImpact with the wall time of its packed encode calls added up."""
    encode_s = 0.0

    def encode_packed_impacts(self, packed):
        t0 = time.perf_counter()
        fmt = super().encode_packed_impacts(packed)
        self.encode_s += time.perf_counter() - t0
        return fmt


REGIONS = ("ib_append", "ib_pair_append", "ib_quantize", "ib_pair_quantize", "ib_scan",
           "ib_compact", "ib_pair_compact", "ib_pair_hist", "ib_pair_scatter", "ib_pair_number",
           "ib_hist", "ib_scatter", "ib_extract")
FILES = ("vocab.txt", "inverted_index.idx", "inverted_index.dat")
BATCH = 400  # passages a batch: one device step on both routes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passages", type=int, default=2000)
    ap.add_argument("--queries", type=int, default=50)
    ap.add_argument("--mean_words", type=int, default=88, help="+ <s> </s>: mean 90 tokens")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--precision", choices=["bf16x3", "fp32"], default="bf16x3")
    ap.add_argument("--pair_bias", type=float, default=0.0, help="as tools/pairwise_e2e.py")
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    a = ap.parse_args()
    torch.cuda.init()
    cfg = EncoderConfig.xlmr_base()
    cfg.activation = "relu"
    sd = bench.synthetic_state_dict(cfg, seed=0)
    w = 0.02 * np.random.default_rng(5).standard_normal(2 * cfg.hidden + 1).astype(np.float32)
    w[0] = 4.0
    sd["pairwise_impact_score_encoder.0.weight"] = torch.from_numpy(w.reshape(1, -1))
    sd["pairwise_impact_score_encoder.0.bias"] = torch.full((1,), a.pair_bias)
    enc = DeviceEncoder(sd, cfg, precision=a.precision)
    model = Timed(enc, local_tokenizer.build_tokenizer(), 512)
    corpus, _ = make_corpus(a.passages, 0, a.mean_words, seed=21)
    texts = list(corpus.values())
    batches = [texts[s:s + BATCH] for s in range(0, len(texts), BATCH)]
    indexer = Indexer(model, model_batch_size=BATCH, num_processes=1)
    tmp = Path(tempfile.mkdtemp(prefix="pair_index_build_ab_"))

    def run(route, n):
        out = tmp / f"{route}{n}"
        model.encode_s = tok_s = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        row = {}
        if route == "text":
            with open(tmp / "collection.index", "w") as f:
                for b in batches:
                    t1 = time.perf_counter()
                    blob = model.pack_processed_blob(model.process_documents(b, model.max_length))
                    tok_s += time.perf_counter() - t1
                    indexer.finish((b, iter([blob])), f, wait=False)
                indexer.drain()
            quantize_file(tmp / "collection.index", tmp / "collection.quantized", sharded=False)
            create_index(tmp / "collection.quantized", out)
            ix = InvertedIndex(out)
        else:
            ix = indexer.build_index(iter(batches), index_path=out)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if route == "text":
            tok, encode = tok_s, model.encode_s
            build = dt - tok - encode
            row["tsv_bytes"] = (tmp / "collection.index").stat().st_size
        else:
            tok, encode, build = (indexer.build_ms[k] / 1e3 for k in ("tokenize", "encode", "build"))
            b = indexer.last_build.builder
            row["regions_ms"] = {r: b.timing(r)[0] for r in REGIONS}
            row["pair_terms"] = int(b.pair_terms()[0].size)
        info = ix.device_index.info()
        row.update({"s": dt, "tokenize_s": tok, "encode_s": encode, "build_s": build,
                    "terms": info["n_terms"], "postings": info["n_postings"]})
        return row, ix, out

    run("direct", "w")
    run("text", "w")
    rows = {"text": [], "direct": []}
    last = {}
    for n in range(a.runs):
        for route in ("text", "direct"):
            row, ix, out = run(route, n)
            rows[route].append(row)
            last[route] = (ix, out)
    files_equal = all((last["text"][1] / f).read_bytes() == (last["direct"][1] / f).read_bytes()
                      for f in FILES)
    rng = np.random.default_rng(5)
    terms = sorted(last["text"][0].vocab)
    queries = [list(rng.choice(terms, int(rng.integers(3, 9)), replace=False))
               for _ in range(a.queries)]
    rank_equal = last["text"][0].score_batch(queries, 1000) == \
        last["direct"][0].score_batch(queries, 1000)

    def summary(rs):
        t = [r["s"] for r in rs]
        med = statistics.median(t)
        out = {"run_s": [round(x, 4) for x in t], "median_s": med, "fastest_s": min(t),
               "spread": (max(t) - min(t)) / med, "terms": rs[0]["terms"],
               "postings": rs[0]["postings"]}
        for k in ("tokenize_s", "encode_s", "build_s"):
            out[k] = statistics.median(r[k] for r in rs)
        return out

    text, direct = summary(rows["text"]), summary(rows["direct"])
    direct["regions_ms"] = {r: statistics.median(x["regions_ms"][r] for x in rows["direct"])
                            for r in REGIONS}
    out = {"tool": "pair_index_build_ab", "precision": a.precision, "passages": a.passages,
           "pair_bias": a.pair_bias, "queries": a.queries, "runs": a.runs, "text_route": text,
           "direct_route": direct, "tsv_bytes": rows["text"][0]["tsv_bytes"],
           "tsv_bytes_per_passage": rows["text"][0]["tsv_bytes"] / a.passages,
           "postings_per_passage": text["postings"] / a.passages,
           "pair_terms": rows["direct"][0]["pair_terms"],
           "text_over_direct": text["median_s"] / direct["median_s"],
           "text_build_over_direct_build": text["build_s"] / direct["build_s"],
           "files_equal": files_equal, "rank_equal": rank_equal,
           "direct_is_faster": direct["median_s"] < text["fastest_s"]}
    shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
