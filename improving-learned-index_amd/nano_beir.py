"""NanoBEIR evaluation path: in-memory sparse search on the GPU.

Reference: src/deep_impact/evaluation/nano_beir_evaluator.py -- SparseSearch
(:70-137) and NanoBEIREvaluator (:153-232).  The model protocol is the
reference's (``get_impact_scores_batch``, ``process_query``), so any model
object the reference accepts works here; the scores are computed by the HIP
float index (di_sparse_*): float32 sums in the reference's order, ties in
first-touch order, bit-exact with the reference under numpy >= 2.

Two routes build the same index (the same bytes on the device, DeviceSparseIndex.export):

  build="device"  the corpus is tokenized once and encoded in steps of up to
      `encode_batch` documents (and the re-ranker's token budget) into a device buffer;
      each step's (term id, impact) pairs are appended from there to a device builder
      (di_sparse_builder_append) and the layout is assembled on the GPU
      (di_sparse_builder_finish): the impacts never visit the host.  Needs a model that
      runs on a DeviceEncoder.
  build="host"  the reference's route, kept as the cross-check: get_impact_scores_batch
      in steps of `encode_batch_size`, a Python list per term, di_sparse_create.

build="auto" takes the device route when the model runs on a DeviceEncoder, else the host
route; DI_SPARSE_HOST_BUILD=1 (environment) forces the host route, for A/B runs.

Datasets: the reference downloads zeta-alpha-ai/Nano* from the hub (:165-167),
which is impossible offline; ``NanoBEIREvaluator`` takes local datasets
(corpus/queries/qrels dicts, or a directory of corpus.jsonl / queries.jsonl /
qrels.tsv).  nDCG follows trec_eval (metrics.ndcg_at_k) since beir/pytrec_eval
are absent (parity unpinned).
"""
from __future__ import annotations

import json
import os
import time
from collections import OrderedDict
from pathlib import Path
from typing import Dict, Optional

import numpy as np

from ._lib import DeviceSparseIndex, SparseBuilder, csr
from .encoder import DeviceEncoder
from .metrics import evaluate_retrieval, ndcg_at_k  # noqa: F401


class SparseSearch:
    def __init__(self, model, batch_size: int, verbose: bool = False, device: int = 0,
                 encode_batch_size: Optional[int] = None, accumulation: str = "f32",
                 build: str = "auto", encode_batch: int = 8192):
        """accumulation: "f32" -- `0.0 + np.float32` under numpy >= 2; "f64" -- under the
        reference's pinned numpy 1.25.1 (f64 doc scores).
        build: "auto" | "device" | "host" (module docstring); encode_batch: documents of
        one encode step of the device route."""
        if accumulation not in ("f32", "f64"):
            raise ValueError(f"accumulation must be 'f32' or 'f64', not {accumulation!r}")
        if build not in ("auto", "device", "host"):
            raise ValueError(f"build must be 'auto', 'device' or 'host', not {build!r}")
        on_device = isinstance(getattr(model, "encoder", None), DeviceEncoder)
        if build == "device" and not on_device:
            raise ValueError("build='device' needs a model that runs on a DeviceEncoder")
        if os.environ.get("DI_SPARSE_HOST_BUILD") == "1":
            build = "host"
        self.build_route = "device" if build == "device" or (build == "auto" and on_device) \
            else "host"
        self.encode_batch = max(1, int(encode_batch))
        # wall time of the device route's build, in ms: tokenize / encode / build
        self.build_ms: Dict[str, float] = {}
        self.accumulation = accumulation
        self.model = model
        self.batch_size = batch_size
        self.encode_batch_size = encode_batch_size or max(batch_size, 256)
        self.verbose = verbose
        self.device = device
        self.inverted_index = None  # DeviceSparseIndex once built
        self.vocab: Dict[str, int] = {}
        self.corpus_ids = []

    def _build_inverted_index(self, corpus):
        """nano_beir_evaluator.py:78-101: terms -> postings in corpus order, score > 0."""
        if self.build_route == "device":
            return self._build_on_device(corpus)
        self.corpus_ids = list(corpus.keys())
        texts = list(corpus.values())
        lists: "OrderedDict[str, list]" = OrderedDict()
        bs = self.encode_batch_size
        for s in range(0, len(texts), bs):
            for di, emb in enumerate(self.model.get_impact_scores_batch(texts[s:s + bs]),
                                     start=s):
                for term, score in emb:
                    if score > 0:
                        lists.setdefault(term, []).append((di, np.float32(score)))
        self.vocab = {t: i for i, t in enumerate(lists)}
        term_off = np.zeros(len(lists) + 1, np.int64)
        term_off[1:] = np.cumsum([len(v) for v in lists.values()])
        pdoc = np.fromiter((d for v in lists.values() for d, _ in v), np.uint32,
                           count=int(term_off[-1]))
        pimp = np.fromiter((x for v in lists.values() for _, x in v), np.float32,
                           count=int(term_off[-1]))
        self.inverted_index = DeviceSparseIndex(term_off, pdoc, pimp, len(self.corpus_ids),
                                                self.device)

    def _build_on_device(self, corpus):
        """_build_inverted_index with the impacts kept on the device: encode steps of up to
        `encode_batch` documents appended to a SparseBuilder.  Term strings are numbered in
        one host table as they appear; `vocab` keeps those that kept a posting (the
        reference's inverted_index has no key for a term whose impacts were all <= 0, and
        an empty term in a query's list would shift the first-touch index of the later
        ones), so its ids need not be dense."""
        import torch

        from .reranker import MAX_STEP_TOKENS

        self.corpus_ids = list(corpus.keys())
        texts = list(corpus.values())
        t0 = time.perf_counter()
        proc = self.model.process_documents(texts, self.model.max_length)
        t_tok = time.perf_counter() - t0
        t_enc = t_build = 0.0
        dev = torch.device("cuda", self.device)
        builder = SparseBuilder(self.device)
        table: Dict[str, int] = {}
        s = 0
        while s < len(proc):
            t0 = time.perf_counter()
            e, tokens = s, 0
            while e < len(proc) and e - s < self.encode_batch and \
                    (e == s or tokens + len(proc[e][0].ids) <= MAX_STEP_TOKENS):
                tokens += len(proc[e][0].ids)
                e += 1
            ids, cu, terms, tt, ct = self.model.pack_processed(proc[s:e])
            tid = np.fromiter((table.setdefault(t, len(table)) for t in terms), np.int64,
                              count=len(terms)).astype(np.uint32).view(np.int32)
            n_terms = len(terms)
            t1 = time.perf_counter()
            d_ids = torch.from_numpy(ids if ids.size else np.zeros(1, np.int32)).to(dev)
            d_cu = torch.from_numpy(cu).to(dev)
            d_tt = torch.from_numpy(tt if tt.size else np.zeros(1, np.int32)).to(dev)
            d_ct = torch.from_numpy(ct).to(dev)
            d_tid = torch.from_numpy(tid if tid.size else np.zeros(1, np.int32)).to(dev)
            d_imp = torch.empty(max(1, n_terms), dtype=torch.float32, device=dev)
            # no ROUND3, as get_impact_scores_batch; synchronous at return (no DI_F_ASYNC):
            # the builder's stream may read d_imp
            self.model.encoder.encode_device(d_ids, d_cu, e - s, int(cu[-1]),
                                             int(np.diff(cu).max(initial=0)), d_tt, d_ct,
                                             n_terms, d_imp)
            t2 = time.perf_counter()
            builder.append(d_tid, d_imp, d_ct, timing=True)
            t3 = time.perf_counter()
            t_build += (t1 - t0) + (t3 - t2)
            t_enc += t2 - t1
            s = e
        t0 = time.perf_counter()
        self.inverted_index = builder.finish(len(table), timing=True)
        builder.close()
        _, blk_off, _, _ = self.inverted_index.export()
        kept = blk_off[:, -1] > 0 if len(table) else np.zeros(0, bool)
        self.vocab = {t: i for (t, i), k in zip(table.items(), kept.tolist()) if k}
        t_build += time.perf_counter() - t0
        self.build_ms = {"tokenize": t_tok * 1e3, "encode": t_enc * 1e3, "build": t_build * 1e3}

    def search(self, queries, corpus, k):
        """nano_beir_evaluator.py:103-137: {qid: {doc_id: float(score)}} in rank order."""
        if self.inverted_index is None:
            self._build_inverted_index(corpus)
        qids = list(queries.keys())
        qterms = [[self.vocab[t] for t in self.model.process_query(queries[q]) if t in self.vocab]
                  for q in qids]
        flat, cu = csr(qterms)
        docs, scores, n, _ = self.inverted_index.search_csr(flat, cu, k,
                                                            accumulation=self.accumulation)
        out = {}
        for i, qid in enumerate(qids):
            out[qid] = {self.corpus_ids[d]: float(s)
                        for d, s in zip(docs[i, :n[i]].tolist(), scores[i, :n[i]].tolist())}
        return out


def _read_local(path: Path):
    corpus, queries, qrels = {}, {}, {}
    with open(path / "corpus.jsonl", encoding="utf-8") as f:
        for line in f:
            x = json.loads(line)
            if len(x["text"]) > 0:
                corpus[x["_id"]] = x["text"]
    with open(path / "queries.jsonl", encoding="utf-8") as f:
        for line in f:
            x = json.loads(line)
            if len(x["text"]) > 0:
                queries[x["_id"]] = x["text"]
    with open(path / "qrels.tsv", encoding="utf-8") as f:
        for line in f:
            p = line.rstrip("\n").split("\t")
            if p[0] == "query-id":
                continue
            qrels.setdefault(p[0], {})[p[1]] = 1
    return corpus, queries, qrels


# nano_beir_evaluator.py:30-60: the 13 NanoBEIR datasets (hub ids zeta-alpha-ai/Nano*)
MAPPING_DATASET_NAME_TO_HUMAN_READABLE = {
    "climatefever": "ClimateFEVER", "dbpedia": "DBPedia", "fever": "FEVER",
    "fiqa2018": "FiQA2018", "hotpotqa": "HotpotQA", "msmarco": "MSMARCO",
    "nfcorpus": "NFCorpus", "nq": "NQ", "quoraretrieval": "QuoraRetrieval",
    "scidocs": "SCIDOCS", "arguana": "ArguAna", "scifact": "SciFact",
    "touche2020": "Touche2020",
}
MAPPING_DATASET_NAME_TO_ID = {k: f"zeta-alpha-ai/Nano{v}"
                              for k, v in MAPPING_DATASET_NAME_TO_HUMAN_READABLE.items()}
K_VALUES = (10, 100, 1000)  # nano_beir_evaluator.py:231


class NanoBEIREvaluator:
    """nano_beir_evaluator.py:153-232 on local data.  A dataset is a (corpus, queries,
    qrels) tuple of dicts or a directory with corpus.jsonl / queries.jsonl / qrels.tsv
    (the hub's NanoBEIR files); ``evaluate_all`` walks ``data_dir``/Nano<Name> for the
    13 datasets (those present) and adds their average as metrics["avg"]."""

    def __init__(self, batch_size=16, verbose=False, device=0, data_dir=None,
                 accumulation="f32", build="auto", encode_batch=8192):
        self.batch_size, self.verbose, self.device = batch_size, verbose, device
        self.accumulation = accumulation
        self.build, self.encode_batch = build, encode_batch
        self.data_dir = Path(data_dir) if data_dir is not None else None

    def _load_dataset(self, dataset):
        if isinstance(dataset, (str, Path)):
            p = Path(dataset)
            if not p.exists() and self.data_dir is not None:
                name = MAPPING_DATASET_NAME_TO_HUMAN_READABLE.get(str(dataset), str(dataset))
                p = self.data_dir / f"Nano{name}"
            return _read_local(p)
        return dataset

    def search(self, model, dataset, k=1000):
        corpus, queries, qrels = self._load_dataset(dataset)
        searcher = SparseSearch(model, batch_size=self.batch_size, verbose=self.verbose,
                                device=self.device, accumulation=self.accumulation,
                                build=self.build, encode_batch=self.encode_batch)
        return searcher.search(queries, corpus, k=k), qrels

    def evaluate_dataset(self, model, dataset):
        """(NDCG, MAP, Recall, P) dicts at k = 10, 100, 1000 (beir's evaluate)."""
        results, qrels = self.search(model, dataset, k=1000)
        return evaluate_retrieval(qrels, results, K_VALUES)

    def evaluate_all(self, model, data_dir=None):
        root = Path(data_dir) if data_dir is not None else self.data_dir
        if root is None:
            raise ValueError("evaluate_all needs data_dir (the hub is unreachable offline)")
        metrics = {}
        for name, human in MAPPING_DATASET_NAME_TO_HUMAN_READABLE.items():
            d = root / f"Nano{human}"
            if not d.is_dir():
                continue
            if self.verbose:
                print(f"Evaluating dataset {name}...")
            metrics[name] = self.evaluate_dataset(model, d)
            if self.verbose:
                print(f"Metrics for {name}: {metrics[name]}")
        if not metrics:
            raise FileNotFoundError(f"no Nano<Name> dataset directory under {root}")
        metrics["avg"] = tuple(
            {key: sum(metrics[n][i][key] for n in metrics) / len(metrics) for key in m}
            for i, m in enumerate(next(iter(metrics.values()))))
        return metrics


def main(argv=None):
    """nano_beir_evaluator.py:236-243 (the reference loads soyuj/deeper-impact from the
    hub; here a local checkpoint + tokenizer and local NanoBEIR directories)."""
    import argparse

    from .models import DeepImpact

    p = argparse.ArgumentParser("NanoBEIR evaluation of a DeepImpact checkpoint.")
    p.add_argument("--data_dir", type=Path, required=True,
                   help="directory holding Nano<Name>/{corpus.jsonl,queries.jsonl,qrels.tsv}")
    p.add_argument("--model_checkpoint_path", type=str, required=True)
    p.add_argument("--tokenizer_path", type=str, default=None)
    p.add_argument("--variant", choices=["xlmr", "bert"], default="bert")
    p.add_argument("--precision", choices=["bf16x3", "fp32", "bf16"], default="bf16x3")
    p.add_argument("--max_length", type=int, default=None)
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--dataset", type=str, default=None, help="one dataset name only")
    p.add_argument("--accumulation", choices=["f32", "f64"], default="f32",
                   help="doc-score sums: f32 (numpy >= 2) or f64 (the reference's numpy 1.25.1)")
    p.add_argument("--build", choices=["auto", "device", "host"], default="auto",
                   help="device: the float index assembled on the GPU from the encoder's device "
                        "output; host: the reference's per-posting route; auto: device when the "
                        "model runs on the HIP encoder")
    p.add_argument("--encode_batch", type=int, default=8192,
                   help="documents of one encode step of the device build")
    a = p.parse_args(argv)
    model = DeepImpact.load(a.model_checkpoint_path, tokenizer_path=a.tokenizer_path,
                            precision=a.precision, device=a.device, variant=a.variant,
                            max_length=a.max_length)
    ev = NanoBEIREvaluator(batch_size=a.batch_size, verbose=True, device=a.device,
                           data_dir=a.data_dir, accumulation=a.accumulation, build=a.build,
                           encode_batch=a.encode_batch)
    out = ev.evaluate_dataset(model, a.dataset) if a.dataset else ev.evaluate_all(model)
    print(out)
    return out


if __name__ == "__main__":
    main()
