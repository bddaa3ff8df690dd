"""Second-stage re-ranking of a top-k run with the DeepImpact encoder (SURVEY §8f F3;
reference src/deep_impact/evaluation/reranker.py:13-91 and src/deep_impact/rerank.py).

For every query of the top-k run, each candidate passage's term impacts are computed
once (the reference's per-pid cache, reranker.py:48-50) and the passage scores
sum(impact of each query term present) in the query-term iteration order
(reranker.py:52-53); the candidates are then sorted by score, stable, first 1000
(reranker.py:91).  The encoder is the same HIP path as indexing (di_encode, float
impacts without the 3-decimal rounding, as compute_term_impacts gives them).

Two routes write the same bytes:

  score="device"  the run is walked in file order in groups of queries; a group closes
      when its not-yet-stored passages reach `encode_batch`.  The group's missing
      passages are tokenized once, encoded in steps of up to `encode_batch` passages (and
      a token budget) into a device buffer and appended from there, with their term ids,
      to a device store of (term id, impact) lists (di_term_store_append): the impacts
      never visit the host.  One di_term_store_score call scores every (query, candidate)
      pair of the group -- float32 adds in the query's term order, as the host sum -- and
      one di_segment_order call orders them (Python's sorted for a query of more than
      DI_MAX_TOPK candidates).
  score="host"  one Python dict per passage, a generator sum per candidate, sorted():
      the literal reference route, kept as the cross-check; passages missing from the
      cache are encoded in batches of `batch_size`.

score="auto" takes the device route when the model runs on a DeviceEncoder, else the
host route; DI_RERANK_HOST=1 (environment) forces the host route, for A/B runs.

Deviation: the device route ignores --batch_size in favour of --encode_batch; batch
boundaries do not change a row's arithmetic, so the bytes stay equal.
"""
from __future__ import annotations

import argparse
import os
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Union

import numpy as np

from . import _lib
from .datasets import Collection, Queries, RunFile, TopKRunFile
from .encoder import DeviceEncoder
from .models import DeepImpact

# tokens of one encode step of the device route: the 8192-document step of the encode
# bench (about 200 tokens a document), which the encoder's workspace is known to hold
MAX_STEP_TOKENS = 8192 * 200


class ReRanker:
    def __init__(self, checkpoint_path: Union[str, Path, None], top_k_run_file_path,
                 queries_path, collection_path, output_path, batch_size: int = 128,
                 num_processes: int = 4, model: Optional[DeepImpact] = None,
                 tokenizer_path=None, precision: str = "bf16x3", device: int = 0,
                 variant: str = "xlmr", max_length: Optional[int] = None,
                 score: str = "auto", encode_batch: int = 8192):
        if score not in ("auto", "device", "host"):
            raise ValueError(f"score must be 'auto', 'device' or 'host', not {score!r}")
        self.top_k = TopKRunFile(run_file_path=top_k_run_file_path)
        self.queries = Queries(queries_path=queries_path)
        self.collection = Collection(collection_path=collection_path)
        self.batch_size = batch_size
        self.encode_batch = max(1, int(encode_batch))
        self.num_processes = num_processes  # tokenization runs in the Rust tokenizer
        self.device = device
        self.model = model if model is not None else DeepImpact.load(
            checkpoint_path, tokenizer_path=tokenizer_path, precision=precision,
            device=device, variant=variant, max_length=max_length)
        self.run_file = RunFile(run_file_path=output_path)
        self.cache: Dict[str, Dict[str, np.float32]] = {}
        on_device = isinstance(getattr(self.model, "encoder", None), DeviceEncoder)
        if score == "device" and not on_device:
            raise ValueError("score='device' needs a model that runs on a DeviceEncoder")
        if os.environ.get("DI_RERANK_HOST") == "1":
            score = "host"
        self.score_route = "device" if score == "device" or (score == "auto" and on_device) \
            else "host"
        # device route: the store, pid -> its store index, term -> its id
        self.store: Optional[_lib.TermStore] = None
        self._doc_of: Dict[str, int] = {}
        self._term_id: Dict[str, int] = {}
        self.encode_ms = 0.0  # wall time inside the device route's encode steps

    # ------------------------------------------------------------------ host route
    def save(self, pids: Sequence[str], batch_doc_term_scores) -> None:
        """reranker.py:48-50."""
        for pid, doc_term_scores in zip(pids, batch_doc_term_scores):
            self.cache[pid] = {term: score for term, score in doc_term_scores}

    def score(self, pid, query_terms):
        """reranker.py:52-53: Python sum from int 0 over the query terms' impacts
        (np.float32 adds under numpy >= 2, as in the reference's environment here)."""
        return sum(self.cache[pid].get(term, 0) for term in query_terms)

    def _encode_missing(self, pids: Sequence[str]) -> None:
        todo = list(dict.fromkeys(p for p in pids if p not in self.cache))
        for s in range(0, len(todo), self.batch_size):
            batch = todo[s:s + self.batch_size]
            self.save(batch, self.model.get_impact_scores_batch([self.collection[p] for p in batch]))

    def _rerank_host(self, qid, pids) -> List:
        query_terms = DeepImpact.process_query(query=self.queries[qid])
        self._encode_missing(pids)
        scores = [self.score(pid, query_terms) for pid in pids]
        return sorted(zip(pids, scores), key=lambda x: x[1], reverse=True)[:1000]

    # ------------------------------------------------------------------ device route
    def _missing(self, pids, seen=None) -> List[str]:
        return [p for p in dict.fromkeys(pids)
                if p not in self._doc_of and (seen is None or p not in seen)]

    def _store_missing(self, pids: Sequence[str]) -> None:
        """ReRanker.save (reranker.py:48-50) on the device: the passages of `pids` (not yet
        stored, distinct) tokenized once, encoded in steps and appended to the store."""
        import time

        import torch

        if self.store is None:
            self.store = _lib.TermStore(self.device)
        if not pids:
            return
        proc = self.model.process_documents([self.collection[p] for p in pids],
                                            self.model.max_length)
        dev = torch.device("cuda", self.device)
        s = 0
        while s < len(pids):
            e, tokens = s, 0
            while e < len(pids) and e - s < self.encode_batch and \
                    (e == s or tokens + len(proc[e][0].ids) <= MAX_STEP_TOKENS):
                tokens += len(proc[e][0].ids)
                e += 1
            ids, cu, terms, tt, ct = self.model.pack_processed(proc[s:e])
            table = self._term_id
            tid = np.fromiter((table.setdefault(t, len(table)) for t in terms), np.int64,
                              count=len(terms)).astype(np.uint32).view(np.int32)
            n_terms = len(terms)
            t0 = time.perf_counter()
            d_ids = torch.from_numpy(ids if ids.size else np.zeros(1, np.int32)).to(dev)
            d_cu = torch.from_numpy(cu).to(dev)
            d_tt = torch.from_numpy(tt if tt.size else np.zeros(1, np.int32)).to(dev)
            d_ct = torch.from_numpy(ct).to(dev)
            d_tid = torch.from_numpy(tid if tid.size else np.zeros(1, np.int32)).to(dev)
            d_imp = torch.empty(max(1, n_terms), dtype=torch.float32, device=dev)
            # synchronous at return (no DI_F_ASYNC): the store's stream may read d_imp
            self.model.encoder.encode_device(d_ids, d_cu, e - s, int(cu[-1]),
                                             int(np.diff(cu).max(initial=0)), d_tt, d_ct,
                                             n_terms, d_imp)
            self.encode_ms += (time.perf_counter() - t0) * 1e3
            first = self.store.append(d_tid, d_imp, d_ct, timing=True)
            for i, p in enumerate(pids[s:e]):
                self._doc_of[p] = first + i
            s = e

    def _rank_device(self, group) -> List[List]:
        """reranker.py:52-53,91 for the (qid, pids) of `group`, whose passages are stored."""
        table = self._term_id
        q_terms, cu_q, cu_c = [], [0], [0]
        for qid, pids in group:
            # the set's iteration order, as the host route; a term no stored passage holds
            # would add the int 0, which changes nothing (the sum starts at +0)
            q_terms += [table[t] for t in DeepImpact.process_query(query=self.queries[qid])
                        if t in table]
            cu_q.append(len(q_terms))
            cu_c.append(cu_c[-1] + len(pids))
        cand = np.fromiter((self._doc_of[p] for _, pids in group for p in pids), np.int32,
                           count=cu_c[-1])
        cu_c = np.asarray(cu_c, np.int32)
        scores, match = self.store.score(np.asarray(q_terms, np.uint32),
                                         np.asarray(cu_q, np.int32), cand, cu_c, timing=True)
        pos = None
        if int(np.diff(cu_c).max(initial=0)) <= _lib.DI_MAX_TOPK:
            pos = _lib.segment_order(scores, cu_c, device=self.device)
        out = []
        for i, (_, pids) in enumerate(group):
            a, b = int(cu_c[i]), int(cu_c[i + 1])
            # Python floats of the float32 sums (RunFile prints a np.float32 through
            # float()); the int 0 where nothing matched, as sum() of no float gives
            sc = [v if m else 0 for v, m in zip(scores[a:b].tolist(), match[a:b].tolist())]
            if pos is None:
                out.append(sorted(zip(pids, sc), key=lambda x: x[1], reverse=True)[:1000])
            else:
                out.append([(pids[j], sc[j]) for j in pos[a:b][:1000].tolist()])
        return out

    # ------------------------------------------------------------------ ranking
    def rerank(self, qid, pids) -> List:
        """reranker.py:56-91."""
        if self.score_route == "host":
            return self._rerank_host(qid, pids)
        self._store_missing(self._missing(pids))
        return self._rank_device([(qid, pids)])[0]

    def run(self) -> None:
        """reranker.py:41-46; on the device route several queries share an encode step,
        a scorer call and an ordering call."""
        if self.score_route == "host":
            for qid, pids in self.top_k:
                self.run_file.writelines(qid, self._rerank_host(qid, pids))
            return
        group, todo, seen = [], [], set()
        for item in list(self.top_k) + [None]:
            if item is not None:
                group.append(item)
                new = self._missing(item[1], seen)
                todo += new
                seen.update(new)
            if group and (item is None or len(todo) >= self.encode_batch):
                self._store_missing(todo)
                for (qid, _), ranked in zip(group, self._rank_device(group)):
                    self.run_file.writelines(qid, ranked)
                group, todo, seen = [], [], set()


def main(argv=None):
    p = argparse.ArgumentParser(
        "Evaluate a DeepImpact model by reranking TopK dataset and computing evaluation metrics.")
    p.add_argument("--checkpoint_path", type=Path, required=True)
    p.add_argument("--top_k_run_file_path", type=Path, required=True)
    p.add_argument("--queries_path", type=Path, required=True)
    p.add_argument("--collection_path", type=Path, required=True)
    p.add_argument("--output_path", type=Path, required=True)
    p.add_argument("--batch_size", type=int, default=128,
                   help="passages of one encode step of the host route (--score host)")
    p.add_argument("--num_processes", type=int, default=4)
    p.add_argument("--tokenizer_path", type=str, default=None)
    p.add_argument("--precision", choices=["bf16x3", "fp32", "bf16"], default="bf16x3",
                   help="bf16x3 (default): fp32-faithful split-bf16; fp32: f32 MFMA; "
                        "bf16: throughput mode, NOT fp32-faithful (different round3 text)")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--variant", choices=["xlmr", "bert"], default="xlmr")
    p.add_argument("--max_length", type=int, default=None)
    p.add_argument("--score", choices=["auto", "device", "host"], default="auto",
                   help="device: impacts kept in a device store, candidates scored and ordered "
                        "on the GPU; host: a dict per passage and Python sums (the reference "
                        "route); auto: device when the model runs on the HIP encoder")
    p.add_argument("--encode_batch", type=int, default=8192,
                   help="passages of one encode step of the device route, across queries")
    args = p.parse_args(argv)
    ReRanker(**vars(args)).run()


if __name__ == "__main__":
    main()
