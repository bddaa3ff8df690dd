"""Device-resident DeeperImpact encoder (ctypes over di_encoder_* / di_encode).

Replaces the reference's model forward + term gather for a batch
(src/deep_impact/models/xlmr_original.py:41-85, :205-225).  PyTorch is used
only to read checkpoints into host tensors.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, Mapping, Optional

import numpy as np

from . import _lib
from ._lib import check, lib, ptr

DI_VARIANT_XLMR, DI_VARIANT_BERT = 0, 1
DI_ACT_SOFTPLUS, DI_ACT_RELU = 0, 1
DI_PREC_BF16, DI_PREC_FP32, DI_PREC_BF16X3 = 0, 1, 2
# "bf16": bf16 MFMA (throughput mode, not fp32-faithful); "fp32": f32 MFMA throughout;
# "bf16x3": split-bf16 GEMMs (3 bf16 products per fp32 product) + f32 attention /
# LayerNorm -- fp32-faithful (impacts within 1e-3 relative of the reference) and fast
PRECISIONS = {"bf16": DI_PREC_BF16, "fp32": DI_PREC_FP32, "bf16x3": DI_PREC_BF16X3}
DI_DTYPE_F32, DI_DTYPE_BF16 = 0, 1
DI_F_ROUND3 = 0x10
DI_F_TOKEN_IMPACTS = 0x20


class di_encoder_cfg(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "variant", "activation", "precision", "vocab_size", "hidden", "layers", "heads",
        "intermediate", "max_positions", "type_vocab", "pad_id")] + [
        ("layer_norm_eps", ctypes.c_float)]


class di_tensor(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("data", ctypes.c_void_p), ("dtype", ctypes.c_int32),
                ("ndim", ctypes.c_int32), ("shape", ctypes.c_int64 * 4)]


@dataclass
class EncoderConfig:
    """Architecture of the checkpoint.  Defaults: xlm-roberta-base, the config
    the reference loads by name (xlmr_original.py:193)."""
    variant: str = "xlmr"          # "xlmr" (RoBERTa positions) | "bert"
    activation: str = "softplus"   # "softplus" (xlmr_original.py:37) | "relu" (original.py:46)
    vocab_size: int = 250002
    hidden: int = 768
    layers: int = 12
    heads: int = 12
    intermediate: int = 3072
    max_positions: int = 514
    type_vocab: int = 1
    pad_id: int = 1
    layer_norm_eps: float = 1e-5

    @classmethod
    def xlmr_base(cls):
        return cls()

    @classmethod
    def bert_base(cls):
        """bert-base-uncased / CoCondenser / soyuj/deeper-impact (ReLU head)."""
        return cls(variant="bert", activation="relu", vocab_size=30522, max_positions=512,
                   type_vocab=2, pad_id=0, layer_norm_eps=1e-12)

    @classmethod
    def from_hf(cls, cfg: Mapping, variant=None, activation=None):
        """From a transformers config dict (config.json)."""
        mt = cfg.get("model_type", "xlm-roberta")
        v = variant or ("bert" if mt == "bert" else "xlmr")
        return cls(variant=v, activation=activation or ("relu" if v == "bert" else "softplus"),
                   vocab_size=cfg["vocab_size"], hidden=cfg["hidden_size"],
                   layers=cfg["num_hidden_layers"], heads=cfg["num_attention_heads"],
                   intermediate=cfg["intermediate_size"],
                   max_positions=cfg["max_position_embeddings"],
                   type_vocab=cfg.get("type_vocab_size", 1),
                   pad_id=cfg.get("pad_token_id", 1 if v == "xlmr" else 0),
                   layer_norm_eps=cfg.get("layer_norm_eps", 1e-5 if v == "xlmr" else 1e-12))

    @classmethod
    def infer(cls, state_dict: Mapping, variant="xlmr", activation=None):
        """Shapes from the state dict, the rest from the variant's base config."""
        base = cls.xlmr_base() if variant == "xlmr" else cls.bert_base()
        if activation:
            base.activation = activation

        def shp(k):
            for p in ("bert.", "roberta.", ""):
                if p + k in state_dict:
                    return tuple(state_dict[p + k].shape)
            raise KeyError(k)

        V, H = shp("embeddings.word_embeddings.weight")
        P = shp("embeddings.position_embeddings.weight")[0]
        T = shp("embeddings.token_type_embeddings.weight")[0]
        F = shp("encoder.layer.0.intermediate.dense.weight")[0]
        L = 0
        while any(f"{p}encoder.layer.{L}.output.dense.weight" in state_dict
                  for p in ("bert.", "roberta.", "")):
            L += 1
        base.vocab_size, base.hidden, base.max_positions = V, H, P
        base.type_vocab, base.intermediate, base.layers = T, F, L
        base.heads = H // 64
        return base

    def to_c(self, precision: str) -> di_encoder_cfg:
        c = di_encoder_cfg()
        c.variant = DI_VARIANT_XLMR if self.variant == "xlmr" else DI_VARIANT_BERT
        c.activation = DI_ACT_SOFTPLUS if self.activation == "softplus" else DI_ACT_RELU
        if precision not in PRECISIONS:
            raise ValueError(f"precision {precision!r}: one of {sorted(PRECISIONS)}")
        c.precision = PRECISIONS[precision]
        for f in ("vocab_size", "hidden", "layers", "heads", "intermediate", "max_positions",
                  "type_vocab", "pad_id"):
            setattr(c, f, getattr(self, f))
        c.layer_norm_eps = self.layer_norm_eps
        return c


def _host_array(t):
    """torch tensor / numpy array -> (contiguous numpy array, DI dtype)."""
    if hasattr(t, "detach"):
        import torch

        t = t.detach().cpu().contiguous()
        if t.dtype == torch.bfloat16:
            return t.view(torch.int16).numpy().view(np.uint16), DI_DTYPE_BF16
        return t.to(torch.float32).numpy(), DI_DTYPE_F32
    a = np.ascontiguousarray(t)
    if a.dtype == np.uint16:
        return a, DI_DTYPE_BF16
    return np.ascontiguousarray(a, np.float32), DI_DTYPE_F32


class DeviceEncoder:
    """Weights resident on one GPU; encode() runs the whole forward there."""

    def __init__(self, state_dict: Mapping, cfg: EncoderConfig, precision="bf16", device=0):
        if precision == "bf16x3" and not (cfg.hidden in (768, 1024) and cfg.intermediate % 256 == 0):
            precision = "fp32"  # split-bf16 kernels take base / large shapes; f32 MFMA otherwise
        self.cfg, self.precision, self.device = cfg, precision, device
        keep, tens = [], []
        for k, v in state_dict.items():
            if not (hasattr(v, "shape") and len(v.shape) <= 4):
                continue
            if hasattr(v, "is_floating_point") and not v.is_floating_point():
                continue  # e.g. embeddings.position_ids (int64 buffer)
            a, dt = _host_array(v)
            name = k.encode("utf-8")
            keep += [a, name]
            t = di_tensor()
            t.name, t.data, t.dtype, t.ndim = name, a.ctypes.data, dt, a.ndim
            for i, d in enumerate(a.shape):
                t.shape[i] = d
            tens.append(t)
        arr = (di_tensor * max(1, len(tens)))(*tens)
        h = ctypes.c_void_p()
        c = cfg.to_c(precision)
        check(lib().di_encoder_create(ctypes.byref(c), arr, len(tens), device, ctypes.byref(h)))
        self._h = h

    def encode_packed(self, ids, cu_seqlens, term_tok=None, cu_terms=None, round3=False,
                      token_impacts=False, timing=False):
        """Host arrays in, host float32 impacts out (per term, or per token)."""
        ids = np.ascontiguousarray(ids, np.int32)
        cu = np.ascontiguousarray(cu_seqlens, np.int32)
        n_docs = len(cu) - 1
        flags = (DI_F_ROUND3 if round3 else 0) | (_lib.DI_F_TIMING if timing else 0)
        if token_impacts:
            flags |= DI_F_TOKEN_IMPACTS
            out = np.zeros(max(1, int(cu[-1])), np.float32)
            tt = np.zeros(1, np.int32)
            ct = np.zeros(n_docs + 1, np.int32)
        else:
            tt = np.ascontiguousarray(term_tok, np.int32)
            ct = np.ascontiguousarray(cu_terms, np.int32)
            out = np.zeros(max(1, int(ct[-1])), np.float32)
            if tt.size == 0:
                tt = np.zeros(1, np.int32)
        if ids.size == 0:
            ids = np.zeros(1, np.int32)
        check(lib().di_encode(self._h, ptr(ids), ptr(cu), n_docs, 0, 0, ptr(tt), ptr(ct), 0,
                              ptr(out), flags))
        n = int(cu[-1]) if token_impacts else int(ct[-1])
        return out[:n]

    def encode_pairwise(self, ids, cu_seqlens, term_tok, cu_terms, round3=False,
                        attentions=False, timing=False, cu_pairs=None):
        """di_encode_pairwise: the term impacts of encode_packed and, for every
        2-combination of a document's terms, DeepPairwiseImpact's pair score
        (pairwise_impact.py:20-95).  term_tok strictly ascending inside each document.
        Host arrays in -> (single float32 [n_terms], pair float32 [n_pairs], cu_pairs int64
        [n_docs + 1][, attn float32 [n_pairs]]); document d's pairs are in
        itertools.combinations order at cu_pairs[d].  (cu_pairs: computed from cu_terms
        unless given; the library checks it either way.)"""
        ids = np.ascontiguousarray(ids, np.int32)
        cu = np.ascontiguousarray(cu_seqlens, np.int32)
        tt = np.ascontiguousarray(term_tok, np.int32)
        ct = np.ascontiguousarray(cu_terms, np.int32)
        n_docs = len(cu) - 1
        T = np.diff(ct.astype(np.int64))
        if cu_pairs is None:
            cu_pairs = np.zeros(n_docs + 1, np.int64)
            cu_pairs[1:] = np.cumsum(T * (T - 1) // 2)
        cu_pairs = np.ascontiguousarray(cu_pairs, np.int64)
        n_terms, n_pairs = int(ct[-1]), max(int(cu_pairs[-1]), 0)
        single = np.zeros(max(1, n_terms), np.float32)
        pair = np.zeros(max(1, n_pairs), np.float32)
        attn = np.zeros(max(1, n_pairs), np.float32) if attentions else None
        flags = (DI_F_ROUND3 if round3 else 0) | (_lib.DI_F_TIMING if timing else 0)
        if tt.size == 0:
            tt = np.zeros(1, np.int32)
        if ids.size == 0:
            ids = np.zeros(1, np.int32)
        check(lib().di_encode_pairwise(self._h, ptr(ids), ptr(cu), n_docs, 0, 0, ptr(tt), ptr(ct),
                                       0, ptr(cu_pairs), 0, ptr(single), ptr(pair), ptr(attn),
                                       flags))
        out = (single[:n_terms], pair[:n_pairs], cu_pairs)
        return out + (attn[:n_pairs],) if attentions else out

    def encode_pairwise_entries(self, ids, cu_seqlens, term_tok, cu_terms, single_pos=None,
                                round3=False, timing=False, out_cap=None):
        """di_encode_pairwise_entries: encode_pairwise followed by the device ordering of
        DeepPairwiseImpact.compute_term_impacts (pairwise_impact.py:98-129); the pair
        scores stay on the device.  term_tok strictly ascending inside each document;
        single_pos: the position in the document's map of every sorted term (None: the
        identity).  Host arrays in -> (cu_out int64 [n_docs + 1], first int32, second
        int32 (-1: a single term), score float32): entry e of document d (cu_out[d] <= e <
        cu_out[d + 1]) is the sorted term first[e] (a global index), or the pair (first[e],
        second[e]).  out_cap: capacity of the entry arrays (default: every pair kept)."""
        ids = np.ascontiguousarray(ids, np.int32)
        cu = np.ascontiguousarray(cu_seqlens, np.int32)
        tt = np.ascontiguousarray(term_tok, np.int32)
        ct = np.ascontiguousarray(cu_terms, np.int32)
        n_docs = len(cu) - 1
        T = np.diff(ct.astype(np.int64))
        cu_pairs = np.zeros(n_docs + 1, np.int64)
        cu_pairs[1:] = np.cumsum(T * (T - 1) // 2)
        n_terms, n_pairs = int(ct[-1]), max(int(cu_pairs[-1]), 0)
        if single_pos is not None:
            single_pos = np.ascontiguousarray(single_pos, np.int32)
            if single_pos.size != n_terms:
                raise ValueError("single_pos: one position per term")
            if n_terms == 0:
                single_pos = None
        cap = n_terms + n_pairs if out_cap is None else int(out_cap)
        cu_out = np.zeros(n_docs + 1, np.int64)
        # (untouched pages cost nothing: the library writes the entries there are)
        first, second = np.empty(max(1, cap), np.int32), np.empty(max(1, cap), np.int32)
        score = np.empty(max(1, cap), np.float32)
        flags = (DI_F_ROUND3 if round3 else 0) | (_lib.DI_F_TIMING if timing else 0)
        if tt.size == 0:
            tt = np.zeros(1, np.int32)
        if ids.size == 0:
            ids = np.zeros(1, np.int32)
        n = ctypes.c_int64(0)
        rc = lib().di_encode_pairwise_entries(
            self._h, ptr(ids), ptr(cu), n_docs, 0, 0, ptr(tt), ptr(ct), 0, ptr(cu_pairs), 0,
            ptr(single_pos), ptr(cu_out), ptr(first), ptr(second), ptr(score), cap,
            ctypes.byref(n), flags)
        _lib._check_entries(rc, n.value)
        return cu_out, first[:n.value], second[:n.value], score[:n.value]

    def encode_device(self, ids, cu_seqlens, n_docs, n_tokens, max_len, term_tok, cu_terms,
                      n_terms, out, flags=_lib.DI_F_DEVICE_PTRS):
        check(lib().di_encode(self._h, ptr(ids), ptr(cu_seqlens), n_docs, n_tokens, max_len,
                              ptr(term_tok), ptr(cu_terms), n_terms, ptr(out), flags))

    def encode_pairwise_device(self, ids, cu_seqlens, n_docs, n_tokens, max_len, term_tok,
                               cu_terms, n_terms, cu_pairs, n_pairs, out_single, out_pair,
                               out_attn=None, flags=_lib.DI_F_DEVICE_PTRS):
        check(lib().di_encode_pairwise(self._h, ptr(ids), ptr(cu_seqlens), n_docs, n_tokens,
                                       max_len, ptr(term_tok), ptr(cu_terms), n_terms,
                                       ptr(cu_pairs), n_pairs, ptr(out_single), ptr(out_pair),
                                       ptr(out_attn), flags))

    def encode_pairs(self, doc_tok, doc_off, qry_tok, qry_off, pair_doc, pair_qry, fmt,
                     out=None, timing=False):
        """di_encode_pairs: the cross-encoder score of every (passage, query part) pair,
        sequences assembled on the device (cross_encoder.py:9-23).  Host numpy arrays in
        -> numpy float32 [n_pairs]; torch device tensors in (all of them, on this
        encoder's device; `out` optional) -> a torch device tensor."""
        n_docs, n_q, n_pairs = len(doc_off) - 1, len(qry_off) - 1, len(pair_doc)
        flags = _lib.DI_F_TIMING if timing else 0
        if _lib._is_device(pair_doc):
            import torch

            if out is None:
                out = torch.empty(max(1, n_pairs), dtype=torch.float32, device=pair_doc.device)
            flags |= _lib.DI_F_DEVICE_PTRS
        else:
            doc_tok = np.ascontiguousarray(doc_tok, np.int32)
            qry_tok = np.ascontiguousarray(qry_tok, np.int32)
            doc_off = np.ascontiguousarray(doc_off, np.int64)
            qry_off = np.ascontiguousarray(qry_off, np.int64)
            pair_doc = np.ascontiguousarray(pair_doc, np.int32)
            pair_qry = np.ascontiguousarray(pair_qry, np.int32)
            out = np.zeros(max(1, n_pairs), np.float32)
        check(lib().di_encode_pairs(self._h, ptr(doc_tok), ptr(doc_off), n_docs, ptr(qry_tok),
                                    ptr(qry_off), n_q, ptr(pair_doc), ptr(pair_qry), n_pairs,
                                    ctypes.byref(fmt), ptr(out), flags))
        return out[:n_pairs]

    def reserve(self, max_tokens, max_docs, max_terms):
        check(lib().di_encoder_reserve(self._h, max_tokens, max_docs, max_terms))

    def set_stream(self, stream_ptr):
        check(lib().di_encoder_set_stream(self._h, ctypes.c_void_p(stream_ptr)))

    def sync(self):
        check(lib().di_encoder_sync(self._h))

    def timing(self, name, reset=False):
        t = _lib.di_timing()
        check(lib().di_encoder_timing(self._h, name.encode(), ctypes.byref(t), int(reset)))
        return t.ms, t.launches

    def close(self):
        if getattr(self, "_h", None):
            lib().di_encoder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def quantize(impacts, max_val=None, bits=8, device=0):
    """di_quantize: int(v * (2^bits-1)/max) with the reference's fp64 arithmetic."""
    v = np.ascontiguousarray(impacts, np.float32)
    out = np.zeros(max(1, v.size), np.int32)
    used = ctypes.c_double(0.0)
    check(lib().di_quantize(ptr(v if v.size else np.zeros(1, np.float32)), v.size,
                            float(max_val) if max_val is not None else -1.0, bits, ptr(out),
                            ctypes.byref(used), device, None, 0))
    return out[:v.size], used.value
