"""DeepImpact model protocol on MI355X -- host-side mirror of the reference class.

Reference: src/deep_impact/models/xlmr_original.py (DeepImpact, XLM-R + Softplus)
and the upstream BERT/CoCondenser variant (src/deep_impact/models/original.py:10,
19,21,155-177, commented there; soyuj/deeper-impact: BertModel + ReLU).

Same names and argument meaning as the reference protocol used by Indexer
(indexer.py:22,33,46,57) and SparseSearch (nano_beir_evaluator.py:93,114):
``load``, ``process_document``, ``process_query``, ``compute_term_impacts``,
``__call__``, ``get_impact_scores``, ``get_impact_scores_batch``.  Tokenization
and term extraction stay on the host (HF ``tokenizers``, batched in Rust); the
forward, the impact head and the first-occurrence gather run in
libdeepimpact_hip.so.  There is no CPU compute fallback.

Not covered: the PhoBERT variant's VnCoreNLP word segmentation
(original.py:29-39,182-194) needs a Java runtime and models that are not part of
this build; its encoder math is the RoBERTa kernel path here.
"""
from __future__ import annotations

import json
import os
import string
from pathlib import Path
from typing import Dict, Iterable, List, Optional, Sequence, Set, Tuple, Union

import numpy as np

from . import _lib
from .encoder import DeviceEncoder, EncoderConfig

PUNCTUATION = set(string.punctuation)


class Encoding:
    """What process_document returns in place of the reference's MockEncoding
    (xlmr_original.py:16-23): ids / attention_mask / type_ids / word_ids of the
    document (unpadded: the device path packs documents without padding)."""

    __slots__ = ("ids", "attention_mask", "type_ids", "word_ids")

    def __init__(self, ids, word_ids):
        self.ids = list(ids)
        self.attention_mask = [1] * len(self.ids)
        self.type_ids = [0] * len(self.ids)
        self.word_ids = list(word_ids)


def load_tokenizer(path_or_obj):
    """A `tokenizers.Tokenizer` from tokenizer.json (or a directory holding one,
    e.g. a local xlm-roberta-base snapshot), or passed through."""
    if path_or_obj is None:
        return None
    if not isinstance(path_or_obj, (str, Path)):
        return path_or_obj
    from tokenizers import Tokenizer

    p = Path(path_or_obj)
    if p.is_dir():
        p = p / "tokenizer.json"
    return Tokenizer.from_file(str(p))


def _normalize(tok, text: str) -> str:
    n = tok.normalizer
    return n.normalize_str(text) if n is not None else text


def _pre_tokenize(tok, text: str) -> List[str]:
    pt = tok.pre_tokenizer
    if pt is None:
        return text.split()
    return [x[0] for x in pt.pre_tokenize_str(text)]


def _first_token_map(word_ids) -> Dict[int, int]:
    """word index -> index of its first token (xlmr_original.py:153-164)."""
    out, prev = {}, None
    for i, w in enumerate(word_ids):
        if w is None:
            continue
        if w != prev:
            out[w] = i
            prev = w
    return out


def _legacy_bert_map(tokens) -> Dict[int, int]:
    """Upstream BERT logic (original.py:162-170, commented there): every token
    after [CLS] that does not start with '##' opens the next term."""
    out, counter = {}, 0
    for i, t in enumerate(tokens[1:], start=1):
        if t.startswith("##"):
            continue
        out[counter] = i
        counter += 1
    return out


class _WordCache:
    """Per-word token cache for the pre-tokenized document encode.  A pre-tokenized
    input is normalized, pre-tokenized and modelled one word at a time, so a word's
    tokens do not depend on its neighbours (except, for a Metaspace pre-tokenizer with
    prepend_scheme "first", on whether it is the first word: two tables); a document's
    encoding is then the template's prefix specials, its words' cached tokens cut to
    max_length - #specials (the tokenizer's right truncation of a single sequence) and
    the suffix specials.  Misses are encoded in one batched call per document batch.
    Checked against encode_batch (tests/test_host_cpu.py) and self-checked on the first
    batch of each process: any difference turns the cache off."""

    MAX_ENTRIES = 1 << 20
    ANCHOR = "a"

    def __init__(self, tok):
        self.tok = tok
        self.first: Dict[str, List[int]] = {}
        self.other: Dict[str, List[int]] = {}
        e = tok.encode([self.ANCHOR], is_pretokenized=True, add_special_tokens=True)
        wid = e.word_ids
        lo = next(i for i, w in enumerate(wid) if w is not None)
        hi = max(i for i, w in enumerate(wid) if w is not None) + 1
        self.prefix, self.suffix = list(e.ids[:lo]), list(e.ids[hi:])
        self.checked = False
        self.ok = True

    def _fill(self, terms_list: Sequence[Sequence[str]]) -> None:
        mf = {t[0] for t in terms_list if t and t[0] not in self.first}
        mo = {w for t in terms_list for w in t[1:] if w not in self.other}
        if not mf and not mo:
            return
        if len(self.first) + len(self.other) + len(mf) + len(mo) > self.MAX_ENTRIES:
            # bounded memory: start over before this batch's fill, which then holds
            # every word the batch looks up
            self.first.clear()
            self.other.clear()
            mf = {t[0] for t in terms_list if t}
            mo = {w for t in terms_list for w in t[1:]}
        tok = self.tok
        trunc = tok.truncation
        tok.no_truncation()  # (a cached word keeps all its tokens)
        try:
            if mf:
                mf = list(mf)
                for w, e in zip(mf, tok.encode_batch([[w] for w in mf], is_pretokenized=True,
                                                     add_special_tokens=False)):
                    self.first[w] = [i for i, x in zip(e.ids, e.word_ids) if x == 0]
            if mo:
                mo = list(mo)
                for w, e in zip(mo, tok.encode_batch([[self.ANCHOR, w] for w in mo],
                                                     is_pretokenized=True,
                                                     add_special_tokens=False)):
                    self.other[w] = [i for i, x in zip(e.ids, e.word_ids) if x == 1]
        finally:
            if trunc is not None:
                tok.enable_truncation(**trunc)

    def encode(self, terms_list: Sequence[Sequence[str]], max_length: int):
        """[(ids, word_ids)] of each document, as encode_batch(..., is_pretokenized=True,
        add_special_tokens=True) under enable_truncation(max_length)."""
        self._fill(terms_list)
        budget = max(max_length - len(self.prefix) - len(self.suffix), 0)
        out = []
        first, other = self.first, self.other
        for terms in terms_list:
            ids = list(self.prefix)
            wids: List[Optional[int]] = [None] * len(ids)
            room = budget
            for i, w in enumerate(terms):
                if room <= 0:
                    break
                tk = first[w] if i == 0 else other[w]
                if len(tk) > room:
                    tk = tk[:room]
                ids.extend(tk)
                wids.extend([i] * len(tk))
                room -= len(tk)
            ids.extend(self.suffix)
            wids.extend([None] * len(self.suffix))
            out.append((ids, wids))
        return out


def _filter_terms(terms: Sequence[str], idx_map: Dict[int, int]) -> Dict[str, int]:
    """Unique, non-punctuation terms whose tokens survived truncation, in
    first-occurrence order (xlmr_original.py:181-187)."""
    out: Dict[str, int] = {}
    for i, t in enumerate(terms):
        if t not in out and t not in PUNCTUATION and i in idx_map:
            out[t] = idx_map[i]
    return out


class DeepImpact:
    """The DeeperImpact model on one MI355X."""

    max_length = 512
    tokenizer = None  # tokenizers.Tokenizer (class-level, like the reference)
    punctuation = PUNCTUATION
    term_mapping = "word_ids"  # or "bert_legacy" (original.py:162-170)

    def __init__(self, encoder: DeviceEncoder, tokenizer=None, max_length: Optional[int] = None):
        self.encoder = encoder
        if tokenizer is not None:
            type(self).set_tokenizer(tokenizer)
        if max_length is not None:
            self.max_length = max_length

    # ------------------------------------------------------------------ tokenizer
    @classmethod
    def set_tokenizer(cls, tok):
        cls.tokenizer = load_tokenizer(tok)

    @classmethod
    def _tok(cls, max_length):
        tok = cls.tokenizer
        if tok is None:
            raise RuntimeError("no tokenizer: call DeepImpact.set_tokenizer(path/to/tokenizer.json)")
        tok.no_padding()
        tok.enable_truncation(max_length)
        return tok

    @classmethod
    def process_query(cls, query: str) -> Set[str]:
        """xlmr_original.py:114-118."""
        tok = cls.tokenizer
        if tok is None:
            raise RuntimeError("no tokenizer set")
        return set(filter(lambda x: x not in cls.punctuation,
                          _pre_tokenize(tok, _normalize(tok, query))))

    @classmethod
    def process_document(cls, document: str, max_length: Optional[int] = None
                         ) -> Tuple[Encoding, Dict[str, int]]:
        """xlmr_original.py:120-189 (unpadded encoding)."""
        return cls.process_documents([document], max_length)[0]

    @classmethod
    def process_documents(cls, documents: Sequence[str], max_length: Optional[int] = None
                          ) -> List[Tuple[Encoding, Dict[str, int]]]:
        """Batched process_document: one multi-threaded tokenizers call."""
        ml = max_length or cls.max_length
        tok = cls._tok(ml)
        terms = [_pre_tokenize(tok, _normalize(tok, d)) for d in documents]
        wc = cls._word_cache(tok) if cls.term_mapping == "word_ids" else None
        if wc is not None:
            enc = wc.encode(terms, ml)
            if not wc.checked:  # first batch of this process: the same as encode_batch?
                wc.checked = True
                ref = tok.encode_batch(terms, is_pretokenized=True, add_special_tokens=True)
                wc.ok = all(list(e.ids) == ids and list(e.word_ids) == wids
                            for e, (ids, wids) in zip(ref, enc))
                if not wc.ok:
                    cls._wcache = None
                    enc = [(e.ids, e.word_ids) for e in ref]
            return [(Encoding(ids, wids), _filter_terms(t, _first_token_map(wids)))
                    for t, (ids, wids) in zip(terms, enc)]
        encs = tok.encode_batch(terms, is_pretokenized=True, add_special_tokens=True)
        out = []
        for t, e in zip(terms, encs):
            if cls.term_mapping == "bert_legacy":
                m = _legacy_bert_map(e.tokens)
            else:
                m = _first_token_map(e.word_ids)
            out.append((Encoding(e.ids, e.word_ids), _filter_terms(t, m)))
        return out

    _wcache = None
    _wcache_tok = None
    word_cache = os.environ.get("DI_TOKEN_CACHE", "1") != "0"

    @classmethod
    def _word_cache(cls, tok):
        """The process's per-word token cache for `tok` (None when disabled or found
        unequal to encode_batch)."""
        if not cls.word_cache:
            return None
        if cls._wcache_tok is not tok:
            cls._wcache_tok = tok
            cls._wcache = _WordCache(tok)
        return cls._wcache if cls._wcache is not None and cls._wcache.ok else None

    @staticmethod
    def compute_term_impacts(documents_term_to_token_index_map: List[Dict[str, int]],
                             outputs) -> List[List[Tuple[str, float]]]:
        """xlmr_original.py:205-225 for [B, S(,1)] per-token impacts."""
        if hasattr(outputs, "detach"):
            outputs = outputs.detach().cpu().numpy()
        imp = np.asarray(outputs)
        if imp.ndim == 3:
            imp = imp[..., 0]
        return [[(t, imp[i][tok]) for t, tok in m.items()]
                for i, m in enumerate(documents_term_to_token_index_map)]

    # ------------------------------------------------------------------ loading
    @classmethod
    def load(cls, checkpoint_path: Optional[Union[str, Path]] = None, *,
             config: Optional[EncoderConfig] = None, tokenizer_path=None,
             precision: str = "bf16x3", device: int = 0, variant: str = "xlmr",
             max_length: Optional[int] = None) -> "DeepImpact":
        """Replaces DeepImpact.load (xlmr_original.py:191-203) + .to(cuda).eval().

        checkpoint_path: a ModelCheckpoint .pt ({'model_state_dict': ...},
        checkpoint.py:72-77), or a local HF model directory (config.json +
        model.safetensors / pytorch_model.bin).  Hub names cannot be fetched
        offline."""
        sd, cfg = _load_weights(checkpoint_path, config, variant)
        enc = DeviceEncoder(sd, cfg, precision=precision, device=device)
        tok = tokenizer_path
        if tok is None and checkpoint_path is not None and Path(checkpoint_path).is_dir() and \
                (Path(checkpoint_path) / "tokenizer.json").exists():
            tok = Path(checkpoint_path) / "tokenizer.json"
        model = cls(enc, tok, max_length)
        # class-level, like the tokenizer: process_document(s) are classmethods
        cls.term_mapping = "bert_legacy" if variant == "bert" else "word_ids"
        return model

    # ------------------------------------------------------------------ forward
    def __call__(self, input_ids, attention_mask, token_type_ids=None):
        """Reference forward protocol (xlmr_original.py:41-54): padded [B, S]
        batch in, per-token impacts [B, S, 1] (float32, host) out.  Padding
        positions (which the reference never reads) are 0."""
        import torch

        ids = np.asarray(input_ids.cpu() if hasattr(input_ids, "cpu") else input_ids)
        mask = np.asarray(attention_mask.cpu() if hasattr(attention_mask, "cpu")
                          else attention_mask).astype(bool)
        lens = mask.sum(1)
        cu = np.zeros(len(lens) + 1, np.int32)
        cu[1:] = np.cumsum(lens)
        packed = ids[mask].astype(np.int32)
        tok = self.encoder.encode_packed(packed, cu, token_impacts=True)
        out = np.zeros(ids.shape, np.float32)
        out[mask] = tok
        return torch.from_numpy(out).unsqueeze(-1)

    def encode_documents(self, documents: Sequence[str], round3: bool = False,
                         max_length: Optional[int] = None) -> List[List[Tuple[str, np.float32]]]:
        """Tokenize, encode and gather a batch: per document the (term, impact)
        list of compute_term_impacts, optionally with round(impact, 3)."""
        proc = self.process_documents(documents, max_length or self.max_length)
        return self.encode_processed(proc, round3)

    @staticmethod
    def pack_processed(proc):
        """process_documents output -> the packed batch of the C ABI: token ids and
        their offsets, the kept terms (flat) with their first-token index and offsets."""
        lens = np.array([len(e.ids) for e, _ in proc], np.int64)
        cu = np.zeros(len(proc) + 1, np.int32)
        cu[1:] = np.cumsum(lens)
        ids = np.fromiter((i for e, _ in proc for i in e.ids), np.int32, count=int(cu[-1]))
        terms = [t for _, m in proc for t in m]
        tt = np.fromiter((t for _, m in proc for t in m.values()), np.int32, count=len(terms))
        ct = np.zeros(len(proc) + 1, np.int32)
        ct[1:] = np.cumsum([len(m) for _, m in proc])
        return ids, cu, terms, tt, ct

    @staticmethod
    def pack_processed_blob(proc):
        """pack_processed with the kept terms as one UTF-8 blob + byte offsets (what a
        tokenizer worker sends back: no per-term objects to unpickle)."""
        ids, cu, terms, tt, ct = DeepImpact.pack_processed(proc)
        enc = [t.encode("utf-8") for t in terms]
        term_off = np.zeros(len(enc) + 1, np.int64)
        if enc:
            term_off[1:] = np.cumsum([len(b) for b in enc])
        return ids, cu, b"".join(enc), term_off, tt, ct

    @staticmethod
    def merge_packed_blobs(parts):
        """Concatenate pack_processed_blob batches (in order) into one: the tokenizer
        workers' small chunks become one device batch (batch sizes never change the
        impacts: every row's arithmetic is independent of the other documents)."""
        if len(parts) == 1:
            return parts[0]
        ids = np.concatenate([p[0] for p in parts])
        tt = np.concatenate([p[4] for p in parts])
        cu, term_off, ct = [np.zeros(1, np.int32)], [np.zeros(1, np.int64)], [np.zeros(1, np.int32)]
        o_tok = o_byte = o_term = 0
        for p in parts:
            cu.append(p[1][1:] + np.int32(o_tok))
            term_off.append(p[3][1:] + np.int64(o_byte))
            ct.append(p[5][1:] + np.int32(o_term))
            o_tok += int(p[1][-1])
            o_byte += int(p[3][-1])
            o_term += int(p[5][-1])
        return (ids, np.concatenate(cu).astype(np.int32), b"".join(p[2] for p in parts),
                np.concatenate(term_off).astype(np.int64), tt, np.concatenate(ct).astype(np.int32))

    def encode_packed_text(self, packed) -> str:
        """A pack_processed_blob batch -> its impact-TSV lines (round3, native
        formatter), without per-term Python objects."""
        return self.encode_packed_impacts(packed)()

    def encode_packed_impacts(self, packed):
        """Encode a pack_processed_blob batch on the device now; return the formatting
        step as a callable (the native formatter, run later -- Indexer overlaps it with
        the next batch's encode)."""
        ids, cu, blob, term_off, tt, ct = packed
        imp = self.encoder.encode_packed(ids, cu, tt, ct, round3=True)
        return lambda: _lib.format_impact_lines_packed(blob, term_off, imp, ct)

    def encode_packed_terms(self, packed, round3=False):
        """Encode a pack_processed batch: per document its (term, impact) list."""
        ids, cu, terms, tt, ct = packed
        imp = self.encoder.encode_packed(ids, cu, tt, ct, round3=round3)
        return [list(zip(terms[ct[i]:ct[i + 1]], imp[ct[i]:ct[i + 1]]))
                for i in range(len(ct) - 1)]

    def encode_processed(self, proc, round3=False):
        return self.encode_packed_terms(self.pack_processed(proc), round3)

    def get_impact_scores(self, document: str) -> List[Tuple[str, np.float32]]:
        """xlmr_original.py:227-241."""
        return self.get_impact_scores_batch([document])[0]

    def get_impact_scores_batch(self, documents: List[str]) -> List[List[Tuple[str, np.float32]]]:
        """xlmr_original.py:243-267 (no rounding)."""
        return self.encode_documents(documents, round3=False)


# --------------------------------------------------------------------------- cross-encoder
def pack_pairs_host(doc_tok, doc_off, qry_tok, qry_off, pair_doc, pair_qry, prefix, suffix,
                    max_length):
    """The pack rule of di_pairs_pack in numpy: sequence p = prefix ++ the first
    max_length - len(prefix) - len(suffix) tokens of (passage pair_doc[p] ++ query part
    pair_qry[p]) ++ suffix -- the tokenizer's right truncation of a single sequence.
    Returns (tok_ids int32, cu_seqlens int32 [n_pairs + 1])."""
    doc_tok, qry_tok = np.asarray(doc_tok, np.int32), np.asarray(qry_tok, np.int32)
    budget = max_length - len(prefix) - len(suffix)
    if budget < 0:
        raise ValueError("max_length is smaller than the number of special tokens")
    pre, suf = np.asarray(prefix, np.int32), np.asarray(suffix, np.int32)
    parts, cu = [], [0]
    for d, q in zip(pair_doc, pair_qry):
        if not (0 <= d < len(doc_off) - 1 and 0 <= q < len(qry_off) - 1):
            raise IndexError("a pair index is outside its token store")
        content = np.concatenate([doc_tok[doc_off[d]:doc_off[d + 1]],
                                  qry_tok[qry_off[q]:qry_off[q + 1]]])[:budget]
        parts += [pre, content, suf]
        cu.append(cu[-1] + len(pre) + len(content) + len(suf))
    ids = np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
    return ids, np.asarray(cu, np.int32)


class TokenStore:
    """Token ids of a list of texts back to back (no special tokens): tok int32,
    off int64 [n + 1]; on the device after to_device()."""

    def __init__(self, encodings_ids: Sequence[Sequence[int]]):
        lens = np.fromiter((len(x) for x in encodings_ids), np.int64, count=len(encodings_ids))
        self.off = np.zeros(len(lens) + 1, np.int64)
        self.off[1:] = np.cumsum(lens)
        self.tok = np.fromiter((t for x in encodings_ids for t in x), np.int32,
                               count=int(self.off[-1]))
        self.d_tok = self.d_off = None

    def __len__(self):
        return len(self.off) - 1

    def to_device(self, device: int):
        import torch

        dev = torch.device("cuda", device)
        self.d_tok = torch.from_numpy(self.tok if self.tok.size else np.zeros(1, np.int32)).to(dev)
        self.d_off = torch.from_numpy(self.off).to(dev)
        return self


class DeepImpactCrossEncoder(DeepImpact):
    """Cross-encoder head on the same encoder (src/deep_impact/models/cross_encoder.py:9-51):
    the impact head applied to token 0 of f'{document} [SEP] {query}'."""

    SEPARATOR = " [SEP] "

    @classmethod
    def process_cross_encoder_document_and_query(cls, document: str, query: str,
                                                 max_length: Optional[int] = None):
        """cross_encoder.py:25-37: the joined string's encoding, unpadded, truncated to
        max_length."""
        return cls._tok(max_length or cls.max_length).encode(f"{document} [SEP] {query}")

    @classmethod
    def process_cross_encoder_documents_and_query(cls, documents: Sequence[str], query: str,
                                                  max_length: Optional[int] = None):
        """cross_encoder.py:39-51."""
        return cls._tok(max_length or cls.max_length).encode_batch(
            [f"{document} [SEP] {query}" for document in documents])

    # ---- split tokenization: each passage and each query once
    @classmethod
    def pair_template(cls, max_length: Optional[int] = None) -> Tuple[List[int], List[int]]:
        """(prefix ids, suffix ids) the tokenizer's post-processor puts around a single
        sequence."""
        tok = cls._tok(max_length or cls.max_length)
        e = tok.encode("a")
        body = [i for i, w in enumerate(e.word_ids) if w is not None]
        return list(e.ids[:body[0]]), list(e.ids[body[-1] + 1:])

    @classmethod
    def tokenize_passages(cls, passages: Sequence[str], max_length: Optional[int] = None
                          ) -> TokenStore:
        """Passage part of a pair: ids(passage.rstrip()), no special tokens.  (A part
        keeps at least the tokens any sequence can take from it.)"""
        tok = cls._tok(max_length or cls.max_length)
        return TokenStore([e.ids for e in tok.encode_batch([p.rstrip() for p in passages],
                                                           add_special_tokens=False)])

    @classmethod
    def tokenize_queries(cls, queries: Sequence[str], max_length: Optional[int] = None
                         ) -> TokenStore:
        """Query part of a pair: ids('[SEP] ' + query) -- the separator is tokenized with
        the query, whose trailing whitespace stays; no special tokens."""
        tok = cls._tok(max_length or cls.max_length)
        return TokenStore([e.ids for e in tok.encode_batch(["[SEP] " + q for q in queries],
                                                           add_special_tokens=False)])

    def pair_format(self, max_length: Optional[int] = None):
        ml = max_length or self.max_length
        pre, suf = self.pair_template(ml)
        return _lib.pair_format(pre, suf, ml)

    def score_pairs(self, doc_store: TokenStore, query_store: TokenStore, pair_doc, pair_qry,
                    max_length: Optional[int] = None, timing: bool = False):
        """Scores of the pairs (doc_store[pair_doc[p]], query_store[pair_qry[p]]), float32
        [n_pairs] -- di_encode_pairs.  Stores that are on the device (to_device) are read
        there and the result is a torch device tensor; otherwise numpy in, numpy out."""
        fmt = self.pair_format(max_length)
        if doc_store.d_tok is not None and query_store.d_tok is not None:
            import torch

            dev = doc_store.d_tok.device
            pd = torch.as_tensor(np.ascontiguousarray(pair_doc, np.int32)).to(dev) \
                if not hasattr(pair_doc, "data_ptr") else pair_doc
            pq = torch.as_tensor(np.ascontiguousarray(pair_qry, np.int32)).to(dev) \
                if not hasattr(pair_qry, "data_ptr") else pair_qry
            return self.encoder.encode_pairs(doc_store.d_tok, doc_store.d_off, query_store.d_tok,
                                             query_store.d_off, pd, pq, fmt, timing=timing)
        return self.encoder.encode_pairs(doc_store.tok, doc_store.off, query_store.tok,
                                         query_store.off, pair_doc, pair_qry, fmt, timing=timing)

    def score_packed(self, ids, cu_seqlens):
        """Token-0 impact of every packed sequence through the per-token forward -- the
        literal reference route (last_hidden_state[:, 0, :], cross_encoder.py:22-23)."""
        cu = np.asarray(cu_seqlens, np.int64)
        if len(cu) <= 1:
            return np.zeros(0, np.float32)
        tok = self.encoder.encode_packed(ids, cu_seqlens, token_impacts=True)
        return tok[cu[:-1]]

    def __call__(self, input_ids, attention_mask, token_type_ids=None):
        """Reference forward protocol (cross_encoder.py:9-23): padded [B, S] batch in,
        scores [B, 1] (float32, host) out.  token_type_ids are accepted and unused, as in
        the reference (original.py:79-84)."""
        import torch

        ids = np.asarray(input_ids.cpu() if hasattr(input_ids, "cpu") else input_ids)
        mask = np.asarray(attention_mask.cpu() if hasattr(attention_mask, "cpu")
                          else attention_mask).astype(bool)
        cu = np.zeros(len(ids) + 1, np.int32)
        cu[1:] = np.cumsum(mask.sum(1))
        n = len(ids)
        out = self.encoder.encode_packed(ids[mask].astype(np.int32), cu,
                                         np.zeros(n, np.int32), np.arange(n + 1, dtype=np.int32))
        return torch.from_numpy(np.array(out, np.float32)).unsqueeze(-1)


# --------------------------------------------------------------------------- pairwise
def round3(x):
    """numpy's round(np.float32, 3) (indexer.py:64) on an array: fl32(rint(fl32(x * 1000))
    / 1000), what DI_F_ROUND3 applies on the device."""
    x = np.asarray(x, np.float32)
    return (np.rint(x * np.float32(1000.0)) / np.float32(1000.0)).astype(np.float32)


def pair_index(a, b, T):
    """Position of the pair (a, b), a < b < T, in itertools.combinations(range(T), 2)."""
    return a * (2 * T - a - 1) // 2 + (b - a - 1)


def pair_ab(j, T):
    """Inverse of pair_index on int64 arrays: (a, b) of the positions j of documents with
    T terms each (T broadcast against j)."""
    j = np.asarray(j, np.int64)
    T = np.broadcast_to(np.asarray(T, np.int64), j.shape)
    s = (2 * T - 1).astype(np.float64)
    a = ((s - np.sqrt(s * s - 8.0 * j)) * 0.5).astype(np.int64)
    a = np.clip(a, 0, np.maximum(T - 2, 0))
    a -= pair_index(a, a + 1, T) > j          # (the float root may be one off either way)
    a += pair_index(a + 1, a + 2, T) <= j
    return a, a + 1 + (j - pair_index(a, a + 1, T))


def pairwise_entries(tt, ct, single, pair, cu_pairs):
    """The order of DeepPairwiseImpact.compute_term_impacts (pairwise_impact.py:98-129) on
    packed arrays: per document its terms in map order, then the pairs whose score does
    not round to 0.000, in combination order over the terms sorted by token index, the
    whole list sorted by raw score descending (stable: ties keep that order).
    tt / ct: the terms' token index in map order and their offsets; single [n_terms] in
    that order; pair [n_pairs] in combination order of the sorted terms.
    Returns (cu_out int64 [n_docs + 1], is_pair bool [n_out], first int64 [n_out], second
    int64 [n_out], score float32 [n_out]): entry e is term `first` (a global term index)
    or the pair (first, second)."""
    tt, ct = np.asarray(tt, np.int64), np.asarray(ct, np.int64)
    single, pair = np.asarray(single, np.float32), np.asarray(pair, np.float32)
    cu_pairs = np.asarray(cu_pairs, np.int64)
    n_docs, n_terms = len(ct) - 1, int(ct[-1])
    T = np.diff(ct)
    tdoc = np.repeat(np.arange(n_docs), T)
    # rank r of document d's sorted terms -> global term index
    by_tok = np.lexsort((tt[:n_terms], tdoc))
    keep = np.flatnonzero(round3(pair) != 0)
    pdoc = np.searchsorted(cu_pairs, keep, side="right") - 1
    j = keep - cu_pairs[pdoc]
    a, b = pair_ab(j, T[pdoc])
    doc = np.concatenate([tdoc, pdoc])
    score = np.concatenate([single[:n_terms], pair[keep]])
    pos = np.concatenate([np.arange(n_terms) - ct[tdoc], T[pdoc] + j])
    order = np.lexsort((pos, -score, doc))
    first = np.concatenate([np.arange(n_terms), by_tok[ct[pdoc] + a]])[order]
    second = np.concatenate([np.zeros(n_terms, np.int64), by_tok[ct[pdoc] + b]])[order]
    cu_out = np.zeros(n_docs + 1, np.int64)
    cu_out[1:] = np.cumsum(np.bincount(doc, minlength=n_docs))
    return cu_out, (order >= n_terms), first, second, score[order]


class DeepPairwiseImpact(DeepImpact):
    """DeepImpact (RoBERTa body, ReLU head) plus the pair head of
    src/deep_impact/models/pairwise_impact.py: every 2-combination of a document's kept
    terms gets relu(Linear(2H+1)([attn, h_a, h_b])) with attn the largest head-mean
    attention probability between the two first tokens over layers and directions.  The
    reference's Indexer holds the pairwise call in a comment (indexer.py:49-54); this
    class runs what that block and the model define."""

    @classmethod
    def load(cls, checkpoint_path=None, *, config: Optional[EncoderConfig] = None,
             tokenizer_path=None, precision: str = "bf16x3", device: int = 0,
             variant: str = "xlmr", max_length: Optional[int] = None) -> "DeepPairwiseImpact":
        """DeepImpact.load with the ReLU head (original.py:41-48) and the two
        pairwise_impact_score_encoder tensors, which the checkpoint must hold."""
        sd, cfg = _load_weights(checkpoint_path, config, variant)
        if config is None:
            cfg.activation = "relu"
        if "pairwise_impact_score_encoder.0.weight" not in sd:
            raise KeyError("the checkpoint has no pairwise_impact_score_encoder")
        enc = DeviceEncoder(sd, cfg, precision=precision, device=device)
        tok = tokenizer_path
        if tok is None and checkpoint_path is not None and Path(checkpoint_path).is_dir() and \
                (Path(checkpoint_path) / "tokenizer.json").exists():
            tok = Path(checkpoint_path) / "tokenizer.json"
        model = cls(enc, tok, max_length)
        cls.term_mapping = "bert_legacy" if variant == "bert" else "word_ids"
        return model

    # ------------------------------------------------------------------ forward
    def __call__(self, input_ids, attention_mask, token_type_ids=None, pairwise_indices=None):
        """Reference forward protocol (pairwise_impact.py:20-42): padded [B, S] batch and
        per document a list of (token a, token b) pairs, a < b, in -> (per-token impacts
        [B, S, 1], per document the pair scores [n, 1], per document the pair attentions
        [n, 1]), float32 host tensors."""
        import torch

        if pairwise_indices is None:
            raise TypeError("pairwise_indices is required")
        single = DeepImpact.__call__(self, input_ids, attention_mask, token_type_ids)
        ids = np.asarray(input_ids.cpu() if hasattr(input_ids, "cpu") else input_ids)
        mask = np.asarray(attention_mask.cpu() if hasattr(attention_mask, "cpu")
                          else attention_mask).astype(bool)
        cu = np.zeros(len(ids) + 1, np.int32)
        cu[1:] = np.cumsum(mask.sum(1))
        toks = [np.unique(np.asarray(p, np.int64).reshape(-1, 2)) for p in pairwise_indices]
        ct = np.zeros(len(ids) + 1, np.int32)
        ct[1:] = np.cumsum([len(t) for t in toks])
        tt = np.concatenate(toks).astype(np.int32) if toks else np.zeros(0, np.int32)
        _, pair, cu_pairs, attn = self.encoder.encode_pairwise(
            ids[mask].astype(np.int32), cu, tt, ct, attentions=True)
        scores, attns = [], []
        for d, p in enumerate(pairwise_indices):
            p = np.asarray(p, np.int64).reshape(-1, 2)
            if (p[:, 0] >= p[:, 1]).any():
                raise ValueError("pairwise_indices: every pair must be (a, b) with a < b")
            a, b = np.searchsorted(toks[d], p[:, 0]), np.searchsorted(toks[d], p[:, 1])
            at = cu_pairs[d] + pair_index(a, b, len(toks[d]))
            scores.append(torch.from_numpy(pair[at].reshape(-1, 1).copy()))
            attns.append(torch.from_numpy(attn[at].reshape(-1, 1).copy()))
        return single, scores, attns

    @staticmethod
    def compute_term_impacts(documents_term_to_token_index_map: List[Dict[str, int]],
                             outputs) -> List[List[Tuple[str, float]]]:
        """pairwise_impact.py:98-129: outputs = (per-token impacts [B, S(, 1)], per document
        the pair scores in combination order of its terms sorted by token index[, the
        attentions])."""
        maps = documents_term_to_token_index_map
        imp, pairs = outputs[0], outputs[1]
        if hasattr(imp, "detach"):
            imp = imp.detach().cpu().numpy()
        imp = np.asarray(imp)
        if imp.ndim == 3:
            imp = imp[..., 0]
        pairs = [np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x,
                            np.float32).reshape(-1) for x in pairs]
        terms = [t for m in maps for t in m]
        tt = np.fromiter((i for m in maps for i in m.values()), np.int64, count=len(terms))
        ct = np.zeros(len(maps) + 1, np.int64)
        ct[1:] = np.cumsum([len(m) for m in maps])
        single = np.array([imp[d][i] for d, m in enumerate(maps) for i in m.values()], np.float32)
        cu_pairs = np.zeros(len(maps) + 1, np.int64)
        cu_pairs[1:] = np.cumsum([len(x) for x in pairs])
        pair = np.concatenate(pairs) if pairs else np.zeros(0, np.float32)
        names, score, cu_out = _pairwise_named(terms, tt, ct, single, pair, cu_pairs)
        return [list(zip(names[cu_out[d]:cu_out[d + 1]], score[cu_out[d]:cu_out[d + 1]]))
                for d in range(len(maps))]

    @staticmethod
    def host_order() -> bool:
        """DI_PAIRWISE_HOST_ORDER=1: order and name the entries on the host
        (pairwise_entries over encode_pairwise's arrays) -- the second answer of the tests
        and of tools/pairwise_e2e.py's A/B; default: the device order
        (di_encode_pairwise_entries) and the native entry formatter."""
        return os.environ.get("DI_PAIRWISE_HOST_ORDER") == "1"

    def _encode_entries(self, ids, cu, terms, tt, ct, round3_):
        """Host path.  Device call on a packed batch -> (names, scores, cu_out) of its
        lines, ordered and named on the host."""
        tt, ct = np.asarray(tt, np.int32), np.asarray(ct, np.int32)
        n_terms = int(ct[-1])
        tdoc = np.repeat(np.arange(len(ct) - 1), np.diff(ct))
        by_tok = np.lexsort((tt[:n_terms], tdoc))  # (the identity for first-occurrence maps)
        s_sorted, pair, cu_pairs = self.encoder.encode_pairwise(ids, cu, tt[:n_terms][by_tok], ct)
        single = np.empty(n_terms, np.float32)
        single[by_tok] = s_sorted
        names, score, cu_out = _pairwise_named(terms, tt, ct, single, pair, cu_pairs)
        return names, (round3(score) if round3_ else score), cu_out

    def _encode_entries_device(self, ids, cu, tt, ct, round3_):
        """Device path.  A packed batch -> (cu_out, first, second, score): the entries in
        their order (di_encode_pairwise_entries), first / second global term indices in
        map order, second -1 for a single term.  Only the entries reach the host."""
        tt, ct = np.asarray(tt, np.int32), np.asarray(ct, np.int32)
        n_terms = int(ct[-1])
        T = np.diff(ct)
        asc = np.ones(n_terms, bool)  # ascending from the term before, or a document's first
        asc[1:] = tt[1:n_terms] > tt[:n_terms - 1]
        asc[ct[:-1][ct[:-1] < n_terms]] = True
        if asc.all():  # first-occurrence maps: map order is token order
            return self.encoder.encode_pairwise_entries(ids, cu, tt[:n_terms], ct, None,
                                                        round3=round3_)
        tdoc = np.repeat(np.arange(len(ct) - 1), T)
        by_tok = np.lexsort((tt[:n_terms], tdoc))
        pos = (by_tok - ct[tdoc]).astype(np.int32)
        cu_out, first, second, score = self.encoder.encode_pairwise_entries(
            ids, cu, tt[:n_terms][by_tok], ct, pos, round3=round3_)
        by32 = by_tok.astype(np.int32)
        return cu_out, by32[first], np.where(second >= 0, by32[np.maximum(second, 0)],
                                              np.int32(-1)).astype(np.int32), score

    def encode_packed_terms(self, packed, round3=False):
        ids, cu, terms, tt, ct = packed
        if self.host_order():
            names, score, cu_out = self._encode_entries(ids, cu, terms, tt, ct, round3)
        else:
            cu_out, first, second, score = self._encode_entries_device(ids, cu, tt, ct, round3)
            names = [terms[f] if s < 0 else f"{terms[f]}|{terms[s]}"
                     for f, s in zip(first.tolist(), second.tolist())]
        return [list(zip(names[cu_out[d]:cu_out[d + 1]], score[cu_out[d]:cu_out[d + 1]]))
                for d in range(len(ct) - 1)]

    def encode_packed_impacts(self, packed):
        ids, cu, blob, term_off, tt, ct = packed
        if not self.host_order():
            cu_out, first, second, score = self._encode_entries_device(ids, cu, tt, ct, True)
            return lambda: _lib.format_entry_lines(blob, term_off, first, second, score, cu_out)
        terms = [blob[term_off[i]:term_off[i + 1]].decode("utf-8")
                 for i in range(len(term_off) - 1)]
        names, score, cu_out = self._encode_entries(ids, cu, terms, tt, ct, True)

        def fmt():
            enc = [t.encode("utf-8") for t in names]
            off = np.zeros(len(enc) + 1, np.int64)
            if enc:
                off[1:] = np.cumsum([len(b) for b in enc])
            return _lib.format_impact_lines_packed(b"".join(enc), off, score, cu_out)

        return fmt


def _pairwise_named(terms, tt, ct, single, pair, cu_pairs):
    """pairwise_entries with the entries' names: the term, or f'{term1}|{term2}'."""
    cu_out, is_pair, first, second, score = pairwise_entries(tt, ct, single, pair, cu_pairs)
    names = [f"{terms[f]}|{terms[s]}" if p else terms[f]
             for p, f, s in zip(is_pair.tolist(), first.tolist(), second.tolist())]
    return names, score, cu_out


# --------------------------------------------------------------------------- weights
def _load_weights(checkpoint_path, config, variant):
    import torch

    if checkpoint_path is None:
        raise ValueError("a checkpoint path is required (hub downloads are unavailable)")
    p = Path(checkpoint_path)
    if not p.exists():
        raise FileNotFoundError(f"{p} does not exist (hub names cannot be fetched offline)")
    if p.is_dir():
        cfg_json = p / "config.json"
        hf_cfg = json.loads(cfg_json.read_text()) if cfg_json.exists() else None
        if (p / "model.safetensors").exists():
            from safetensors.torch import load_file

            sd = load_file(str(p / "model.safetensors"))
        else:
            sd = torch.load(p / "pytorch_model.bin", map_location="cpu", weights_only=True)
        if config is None and hf_cfg is not None:
            config = EncoderConfig.from_hf(hf_cfg, variant=variant)
    else:
        ck = torch.load(p, map_location="cpu", weights_only=True)
        sd = ck["model_state_dict"] if isinstance(ck, dict) and "model_state_dict" in ck else ck
    if config is None:
        config = EncoderConfig.infer(sd, variant=variant)
    return sd, config
