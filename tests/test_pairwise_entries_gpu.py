"""di_encode_pairwise_entries on the GPU: the encoder's forward followed by the device
ordering of DeepPairwiseImpact.compute_term_impacts (reference pairwise_impact.py:98-129),
against models.pairwise_entries applied to di_encode_pairwise's arrays -- bit-equal, with and
without round3 -- and the text of the pairwise indexer's packed path with the device order
against the host order (DI_PAIRWISE_HOST_ORDER=1).  The seeded encoder_xlmr_small.json
encoder with the pair head of test_pairwise_gpu.py, in fp32 and bf16x3; and a BERT-variant
model, whose map is built by the legacy counter (original.py:162-170)."""
import functools
import json

import numpy as np
import pytest
import torch

import encoder_ref
import pairwise_cases as P
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DOCS = [
    "the learned sparse retrieval model computes an impact score",
    "search engines index passages and queries hit the inverted index",
    "a very long passage about water and earth and the sea",
    "hello world it is ok",
    "the model computes a score about water",
    "queries about the sea and the earth",
    "sparse retrieval of passages",
    "single",
    "",
    "ok ok ok world",
    "water water water",
    "the sea, the earth; the world: hello (ok)",
    "numbers and symbols and text about retrieval of the impact of the model",
]


def _pair_head(sd, H):
    w = np.random.default_rng(P.PAIR_SEED).standard_normal(2 * H + 1) * 0.05
    w[0] = 4.0
    sd["pairwise_impact_score_encoder.0.weight"] = torch.from_numpy(
        w.astype(np.float32).reshape(1, -1))
    sd["pairwise_impact_score_encoder.0.bias"] = torch.zeros(1)
    return sd


@functools.lru_cache(maxsize=None)
def xlmr_checkpoint():
    fx = json.loads((GOLDEN / "encoder_xlmr_small.json").read_text())
    sd = encoder_ref.seeded_state_dict(fx["state_dict_shapes"], fx["seed"], fx["std"])
    return _pair_head(sd, fx["config"]["hidden_size"]), fx["max_length"]


@pytest.fixture
def model_class():
    """DeepPairwiseImpact with the class-level tokenizer state put back afterwards."""
    from improving_learned_index_amd import _lib, models

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible (GPU test run without a GPU)")
    classes, keys = (models.DeepImpact, models.DeepPairwiseImpact), ("tokenizer", "term_mapping",
                                                                     "max_length")
    saved = [{k: c.__dict__[k] for k in keys if k in c.__dict__} for c in classes]
    yield models.DeepPairwiseImpact
    for c, was in zip(classes, saved):
        for k in keys:
            if k in was:
                setattr(c, k, was[k])
            elif k in c.__dict__:
                delattr(c, k)


def _xlmr(model_class, tmp_path, prec):
    sd, max_length = xlmr_checkpoint()
    ckpt = tmp_path / "DeepPairwiseImpact_latest.pt"
    torch.save({"model_state_dict": sd}, ckpt)
    return model_class.load(ckpt, tokenizer_path=GOLDEN / "tokenizer.json", precision=prec,
                            max_length=max_length), max_length


def _entries_equal(enc, ids, cu, tt, ct, pos, round3_):
    """encode_pairwise_entries against pairwise_entries over encode_pairwise's arrays;
    tt ascending inside each document, pos the terms' map positions (None: identity)."""
    from improving_learned_index_amd.models import pairwise_entries, round3

    single, pair, cup = enc.encode_pairwise(ids, cu, tt, ct)
    n = int(ct[-1])
    doc0 = np.repeat(ct[:-1].astype(np.int64), np.diff(ct))
    bt = doc0 + (np.arange(n) - doc0 if pos is None else pos.astype(np.int64))
    tt_map, s_map = np.empty(n, np.int64), np.empty(n, np.float32)
    tt_map[bt], s_map[bt] = tt, single
    wcu, wpair, wfirst, wsecond, wscore = pairwise_entries(tt_map, ct, s_map, pair, cup)
    got_cu, first, second, score = enc.encode_pairwise_entries(ids, cu, tt, ct, pos,
                                                               round3=round3_)
    assert got_cu.tolist() == wcu.tolist() and len(first) == wcu[-1]
    assert ((second >= 0) == wpair).all()
    assert (bt[first] == wfirst).all() and (bt[second[wpair]] == wsecond[wpair]).all()
    assert (second[~wpair] == -1).all()
    want = round3(wscore) if round3_ else wscore
    assert score.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    return got_cu, first, second, score, pair


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_entries_equal_pairwise_entries_of_the_encoders_arrays(model_class, tmp_path, prec):
    model, max_length = _xlmr(model_class, tmp_path, prec)
    proc = model.process_documents(DOCS, max_length)
    ids, cu, terms, tt, ct = model.pack_processed(proc)
    rng = np.random.default_rng(3)
    perm = np.concatenate([rng.permutation(int(t)) for t in np.diff(ct)]).astype(np.int32)
    for pos in (None, perm):
        for r3 in (False, True):
            out = _entries_equal(model.encoder, ids, cu, tt, ct, pos, r3)
    cu_out, first, second, score, pair = out
    n_pairs_kept = int((second >= 0).sum())
    assert 0 < n_pairs_kept < len(pair)  # some pairs are kept, some round to 0.000
    assert (np.diff(cu_out)[np.diff(ct) == 0] == 0).all() and (np.diff(ct) == 0).any()


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_packed_text_equals_the_host_order(model_class, tmp_path, prec, monkeypatch):
    model, max_length = _xlmr(model_class, tmp_path, prec)
    proc = model.process_documents(DOCS, max_length)
    packed = model.pack_processed_blob(proc)
    monkeypatch.delenv("DI_PAIRWISE_HOST_ORDER", raising=False)
    device_text = model.encode_packed_impacts(packed)()
    device_terms = model.encode_packed_terms(model.pack_processed(proc), round3=True)
    monkeypatch.setenv("DI_PAIRWISE_HOST_ORDER", "1")
    host_text = model.encode_packed_impacts(packed)()
    host_terms = model.encode_packed_terms(model.pack_processed(proc), round3=True)
    assert device_text == host_text
    assert device_text.count("\n") == len(DOCS) and "|" in device_text
    assert device_text == P.restated_lines(host_terms)
    assert [[(t, v.tobytes()) for t, v in d] for d in device_terms] == \
           [[(t, v.tobytes()) for t, v in d] for d in host_terms]


def test_second_call_after_the_workspace_grew(model_class, tmp_path):
    model, max_length = _xlmr(model_class, tmp_path, "fp32")
    small = model.pack_processed(model.process_documents(DOCS[:2], max_length))
    big = model.pack_processed(model.process_documents(DOCS * 3, max_length))

    def entries(p):
        ids, cu, _, tt, ct = p
        return [a.copy() for a in model.encoder.encode_pairwise_entries(ids, cu, tt, ct,
                                                                         round3=True)]

    first_small = entries(small)
    first_big = entries(big)  # grows every buffer of the workspace
    for a, b in zip(first_small, entries(small)):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(first_big, entries(big)):
        assert a.tobytes() == b.tobytes()
    n = len(DOCS)
    cu_out = first_big[0]  # the batch holds DOCS three times: three equal thirds
    assert (np.diff(cu_out)[:n] == np.diff(cu_out)[n:2 * n]).all()
    assert first_big[3][:cu_out[n]].tobytes() == first_big[3][cu_out[n]:cu_out[2 * n]].tobytes()
    # a capacity too small: DI_ERANGE with the entries needed, and the next call is right
    from improving_learned_index_amd import _lib
    ids, cu, _, tt, ct = small
    with pytest.raises(_lib.DIError) as e:
        model.encoder.encode_pairwise_entries(ids, cu, tt, ct, out_cap=3)
    assert e.value.code == _lib.DI_ERANGE and e.value.needed == len(first_small[1])
    for a, b in zip(first_small, entries(small)):
        assert a.tobytes() == b.tobytes()


def test_bert_variant_map_order(model_class, tmp_path, monkeypatch):
    """variant "bert": absolute positions and the legacy counter's map.  The text of the
    device path equals the host path's; so do the entries of a batch whose map order is
    not token order (the single_pos route of the model)."""
    from test_encoder_bert_gpu import BERT_BASE, _bert_tokenizer, _shapes

    rng = np.random.default_rng(5)
    words = [f"w{i}" for i in range(120)]
    n_vocab = _bert_tokenizer(tmp_path / "tokenizer.json", words)
    c = dict(BERT_BASE, vocab_size=n_vocab, num_hidden_layers=2)
    sd = encoder_ref.seeded_state_dict(_shapes(c), seed=7, std=0.02)
    sd["impact_score_encoder.0.bias"] = torch.tensor([0.05])
    _pair_head(sd, c["hidden_size"])
    ckpt = tmp_path / "DeepPairwiseImpact_latest.pt"
    torch.save({"model_state_dict": sd}, ckpt)
    model = model_class.load(ckpt, tokenizer_path=tmp_path / "tokenizer.json",
                             precision="bf16x3", variant="bert", max_length=48)
    assert model_class.term_mapping == "bert_legacy"
    docs = [" ".join(words[int(x)] + ("s" if rng.random() < 0.2 else "")
                     for x in rng.integers(0, 120, int(rng.integers(3, 60)))) + ", ok."
            for _ in range(12)]
    proc = model.process_documents(docs, 48)
    packed = model.pack_processed_blob(proc)
    monkeypatch.delenv("DI_PAIRWISE_HOST_ORDER", raising=False)
    device_text = model.encode_packed_impacts(packed)()
    # the same documents with every map reversed: the map order is no longer token order
    ids, cu, terms, tt, ct = model.pack_processed(proc)
    rev = np.concatenate([np.arange(ct[d + 1] - 1, ct[d] - 1, -1) for d in range(len(docs))])
    r_terms, r_tt = [terms[i] for i in rev], tt[rev]
    assert (np.diff(r_tt[ct[0]:ct[1]]) < 0).all()
    device_rev = model.encode_packed_terms((ids, cu, r_terms, r_tt, ct), round3=True)
    monkeypatch.setenv("DI_PAIRWISE_HOST_ORDER", "1")
    assert device_text == model.encode_packed_impacts(packed)()
    assert "|" in device_text and device_text.count("\n") == len(docs)
    host_rev = model.encode_packed_terms((ids, cu, r_terms, r_tt, ct), round3=True)
    assert [[(t, v.tobytes()) for t, v in d] for d in device_rev] == \
           [[(t, v.tobytes()) for t, v in d] for d in host_rev]
    assert any(a != b for a, b in zip(device_rev, model.encode_packed_terms(
        (ids, cu, terms, tt, ct), round3=True)))  # (the reversal changed the tie order)
