"""Cross-encoder re-ranking of a top-k file on the HIP encoder (reference
src/deep_impact/evaluation/cross_encoder_reranker.py:12-62 and
src/deep_impact/cross_encoder_rerank.py).

For every query of the TopKDataset, each candidate passage is scored by the impact head
on token 0 of f'{passage} [SEP] {query}' (src/deep_impact/models/cross_encoder.py:22-23,
37) and the candidates are written in the order of
sorted(zip(pids, scores), key=lambda x: x[1], reverse=True) -- every candidate, no cut
(cross_encoder_reranker.py:36,62).

Two routes compute the same scores:

  assemble="device" (default)  every unique passage and every query is tokenized once
      (DeepImpactCrossEncoder.tokenize_passages / tokenize_queries), the two token stores
      are uploaded once, and the sequences are assembled on the GPU from pair indices
      (di_encode_pairs); the order comes from di_segment_order (Python's sorted for a
      query of more than DI_MAX_TOPK candidates).  The first device step of a run is
      also tokenized joined on the host; if any sequence differs, the whole run takes the
      joined route (the safeguard _WordCache.checked applies to documents).
  assemble="joined"  the joined strings are tokenized on the host and scored through the
      per-token forward, token 0 taken: the literal reference route, kept as the
      cross-check and the fallback.

Deviation: --batch_size is the number of pairs of one device step, across queries (the
reference batches inside one query, default 32), bounded also by a token budget; a
sequence's score does not depend on the batch it is in.
"""
from __future__ import annotations

import argparse
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from .datasets import Collection, RunFile, TopKDataset
from .models import DeepImpactCrossEncoder, pack_pairs_host

MAX_STEP_TOKENS = 1 << 17  # tokens of one device step (the encoder's workspace grows with it)


def _resolve_tokenizer(checkpoint_path, tokenizer_path):
    """The explicit path, else a tokenizer.json in (or next to) the checkpoint."""
    if tokenizer_path is not None or checkpoint_path is None:
        return tokenizer_path
    p = Path(checkpoint_path)
    for cand in ((p / "tokenizer.json") if p.is_dir() else None, p.parent / "tokenizer.json"):
        if cand is not None and cand.exists():
            return cand
    return None


class CrossEncoderReRanker:
    def __init__(self, checkpoint_path: Union[str, Path, None], top_k_path, collection_path,
                 output_path, batch_size: int = 2048,
                 model: Optional[DeepImpactCrossEncoder] = None, tokenizer_path=None,
                 precision: str = "bf16x3", device: int = 0, variant: str = "xlmr",
                 max_length: Optional[int] = None, assemble: str = "device"):
        if assemble not in ("device", "joined"):
            raise ValueError(f"assemble must be 'device' or 'joined', not {assemble!r}")
        self.top_k = TopKDataset(top_k_path=top_k_path)
        self.collection = Collection(collection_path=collection_path)
        self.batch_size = max(1, int(batch_size))
        self.device = device
        self.model = model if model is not None else DeepImpactCrossEncoder.load(
            checkpoint_path, tokenizer_path=_resolve_tokenizer(checkpoint_path, tokenizer_path),
            precision=precision, device=device, variant=variant, max_length=max_length)
        self.max_length = max_length or self.model.max_length
        self.run_file = RunFile(run_file_path=output_path)
        self.assemble = assemble
        self._stores = None
        self._checked = False

    # ------------------------------------------------------------------ joined route
    def _score_joined(self, pairs: Sequence[Tuple[str, str]]) -> np.ndarray:
        """Scores of (qid, pid) pairs: joined strings tokenized on the host
        (cross_encoder_reranker.py:52-59), token 0 of the per-token forward."""
        out = np.zeros(len(pairs), np.float32)
        s = 0
        while s < len(pairs):
            ids, cu = [], [0]
            e = s
            while e < len(pairs) and e - s < self.batch_size:
                qid, pid = pairs[e]
                enc = DeepImpactCrossEncoder.process_cross_encoder_document_and_query(
                    self.collection[pid], self.top_k.queries[qid], self.max_length)
                if e > s and cu[-1] + len(enc.ids) > MAX_STEP_TOKENS:
                    break
                ids += enc.ids
                cu.append(cu[-1] + len(enc.ids))
                e += 1
            out[s:e] = self.model.score_packed(np.asarray(ids, np.int32),
                                               np.asarray(cu, np.int32))
            s = e
        return out

    # ------------------------------------------------------------------ device route
    def _build_stores(self):
        """Every candidate passage and every query tokenized once; stores on the device."""
        pids = list(dict.fromkeys(p for qid in self.top_k.keys() for p in self.top_k[qid]))
        qids = list(self.top_k.keys())
        docs = DeepImpactCrossEncoder.tokenize_passages([self.collection[p] for p in pids],
                                                        self.max_length)
        qrys = DeepImpactCrossEncoder.tokenize_queries([self.top_k.queries[q] for q in qids],
                                                       self.max_length)
        import torch

        docs.to_device(self.device)
        qrys.to_device(self.device)
        torch.cuda.synchronize(self.device)
        self._stores = (docs, qrys, {p: i for i, p in enumerate(pids)},
                        {q: i for i, q in enumerate(qids)})
        pre, suf = DeepImpactCrossEncoder.pair_template(self.max_length)
        self._n_fixed = len(pre) + len(suf)
        self._template = (pre, suf)

    def _split_equals_joined(self, pairs, pd, pq) -> bool:
        """The split stores packed by the pack rule == the joined strings' encodings?"""
        docs, qrys = self._stores[0], self._stores[1]
        pre, suf = self._template
        ids, cu = pack_pairs_host(docs.tok, docs.off, qrys.tok, qrys.off, pd, pq, pre, suf,
                                  self.max_length)
        for i, (qid, pid) in enumerate(pairs):
            enc = DeepImpactCrossEncoder.process_cross_encoder_document_and_query(
                self.collection[pid], self.top_k.queries[qid], self.max_length)
            if list(enc.ids) != ids[cu[i]:cu[i + 1]].tolist():
                return False
        return True

    def _score_device(self, pairs: Sequence[Tuple[str, str]]):
        """Scores of (qid, pid) pairs as a torch device tensor, or None when the
        first-step check found the split tokenization unequal to the joined one."""
        import torch

        if self._stores is None:
            self._build_stores()
        docs, qrys, pidx, qidx = self._stores
        pd = np.fromiter((pidx[p] for _, p in pairs), np.int32, count=len(pairs))
        pq = np.fromiter((qidx[q] for q, _ in pairs), np.int32, count=len(pairs))
        budget = self.max_length - self._n_fixed
        lens = np.minimum((docs.off[pd + 1] - docs.off[pd]) + (qrys.off[pq + 1] - qrys.off[pq]),
                          budget) + self._n_fixed
        out = torch.empty(max(1, len(pairs)), dtype=torch.float32,
                          device=torch.device("cuda", self.device))
        s = 0
        while s < len(pairs):
            e, tokens = s, 0
            while e < len(pairs) and e - s < self.batch_size and \
                    (e == s or tokens + int(lens[e]) <= MAX_STEP_TOKENS):
                tokens += int(lens[e])
                e += 1
            if not self._checked:  # first device step of this run
                self._checked = True
                if not self._split_equals_joined(pairs[s:e], pd[s:e], pq[s:e]):
                    return None
            out[s:e] = self.model.score_pairs(docs, qrys, pd[s:e], pq[s:e], self.max_length)
            s = e
        return out[:len(pairs)]

    # ------------------------------------------------------------------ ranking
    def _rank(self, qids: Sequence[str]) -> Dict[str, List[Tuple[str, float]]]:
        """cross_encoder_reranker.py:41-62 for several queries in one go."""
        pairs = [(qid, pid) for qid in qids for pid in self.top_k[qid]]
        cu = np.zeros(len(qids) + 1, np.int32)
        cu[1:] = np.cumsum([len(self.top_k[qid]) for qid in qids])
        scores_d = self._score_device(pairs) if self.assemble == "device" else None
        if scores_d is None:
            self.assemble = "joined"
            scores = self._score_joined(pairs)
            pos = None
        else:
            import torch

            pos = None
            if int(np.diff(cu).max(initial=0)) <= _lib.DI_MAX_TOPK:
                pos = _lib.segment_order(scores_d, torch.from_numpy(cu).to(scores_d.device),
                                         device=self.device).cpu().numpy()
            scores = scores_d.cpu().numpy()
        out = {}
        for i, qid in enumerate(qids):
            pids = self.top_k[qid]
            sc = scores[cu[i]:cu[i + 1]].tolist()  # Python floats of the float32 scores
            if pos is None:
                out[qid] = sorted(zip(pids, sc), key=lambda x: x[1], reverse=True)
            else:
                out[qid] = [(pids[j], sc[j]) for j in pos[cu[i]:cu[i + 1]]]
        return out

    def rerank(self, qid, pbar=None) -> List[Tuple[str, float]]:
        """cross_encoder_reranker.py:41-62: the query's candidates by score, descending,
        equal scores in file order."""
        return self._rank([str(qid)])[str(qid)]

    def run(self) -> None:
        """cross_encoder_reranker.py:34-39: queries in top_k.keys() order; several queries
        share a device step."""
        group, n = [], 0
        for qid in list(self.top_k.keys()) + [None]:
            if qid is not None:
                group.append(qid)
                n += len(self.top_k[qid])
            if group and (qid is None or n >= self.batch_size):
                ranked = self._rank(group)
                for g in group:
                    self.run_file.writelines(g, ranked[g])
                group, n = [], 0


def main(argv=None):
    p = argparse.ArgumentParser(
        "Evaluate a Cross Encoder DeepImpact model by reranking TopK dataset.")
    p.add_argument("--checkpoint_path", type=Path, required=True)
    p.add_argument("--top_k_path", type=Path, required=True)
    p.add_argument("--collection_path", type=Path, required=True)
    p.add_argument("--output_path", type=Path, required=True)
    p.add_argument("--batch_size", type=int, default=2048,
                   help="pairs of one device step, across queries (reference: 32 per query)")
    p.add_argument("--tokenizer_path", type=str, default=None,
                   help="default: tokenizer.json in or next to the checkpoint")
    p.add_argument("--precision", choices=["bf16x3", "fp32", "bf16"], default="bf16x3",
                   help="bf16x3 (default): fp32-faithful split-bf16; fp32: f32 MFMA; "
                        "bf16: throughput mode, NOT fp32-faithful")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--variant", choices=["xlmr", "bert"], default="xlmr")
    p.add_argument("--max_length", type=int, default=None)
    p.add_argument("--assemble", choices=["device", "joined"], default="device",
                   help="device: sequences assembled on the GPU from token stores; joined: "
                        "joined strings tokenized on the host (the reference route)")
    args = p.parse_args(argv)
    CrossEncoderReRanker(**vars(args)).run()


if __name__ == "__main__":
    main()
