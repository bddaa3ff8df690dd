"""CPU checks of the cross-encoder reranker's host side: the TopKDataset loader against
the reference's own (tests/golden/make_golden_cross.py), the split tokenization rule
(passage and query tokenized once each) against the joined string the reference
tokenizes (src/deep_impact/models/cross_encoder.py:37,51), and the pack rule of
di_pairs_pack restated in numpy against hand-written sequences."""
import json

import numpy as np
import pytest

import cross_cases as C
import local_tokenizer
from conftest import GOLDEN


# ------------------------------------------------------------------ TopKDataset
def test_topk_dataset_matches_reference_loader():
    from improving_learned_index_amd.datasets import TopKDataset

    want = json.loads((GOLDEN / "topk_dataset.json").read_text(encoding="utf-8"))
    ds = TopKDataset(top_k_path=GOLDEN / "topk_fixture.tsv")
    assert ds.queries == want["queries"] and list(ds.queries) == list(want["queries"])
    assert ds.passages == want["passages"] and list(ds.passages) == list(want["passages"])
    assert ds.top_k == want["top_k"]
    assert list(ds.keys()) == want["keys"]
    assert len(ds) == want["len"]
    assert (ds.min_len, ds.max_len, ds.avg_len) == (want["min_len"], want["max_len"],
                                                    want["avg_len"])
    for qid, pids in want["getitem"].items():
        assert ds[qid] == pids
    assert ds[7] == want["getitem"]["7"]  # __getitem__ takes str(qid)


def test_topk_dataset_assertions_fire(tmp_path):
    from improving_learned_index_amd.datasets import TopKDataset

    dup = tmp_path / "dup.tsv"
    dup.write_text("1\t5\tq one\tp five\n1\t6\tq one\tp six\n1\t5\tq one\tp five\n")
    with pytest.raises(AssertionError, match="TopK file contains duplicates"):
        TopKDataset(dup)
    mis = tmp_path / "mis.tsv"
    mis.write_text("1\t5\tq one\tp five\n1\t6\tq other\tp six\n")
    with pytest.raises(AssertionError, match="TopK file is not in the expected format"):
        TopKDataset(mis)


# ------------------------------------------------------------------ split vs joined
@pytest.fixture(scope="module")
def text_pairs():
    return C.seeded_text_pairs(2000, seed=5)


@pytest.mark.parametrize("which", ["unigram", "wordpiece"])
def test_split_tokenization_equals_joined(which, text_pairs):
    """ids(passage.rstrip()) ++ ids('[SEP] ' + query) packed by the pack rule == the ids
    of f'{passage} [SEP] {query}' under enable_truncation(max_length): 0 mismatches over
    2000 seeded pairs (max_length 40 puts the cut inside many passages and queries)."""
    from improving_learned_index_amd.models import DeepImpactCrossEncoder as X
    from improving_learned_index_amd.models import pack_pairs_host

    tok = local_tokenizer.build_tokenizer() if which == "unigram" \
        else C.build_wordpiece_tokenizer()
    saved = X.tokenizer
    X.set_tokenizer(tok)
    try:
        for ml in (40, 512):
            pre, suf = X.pair_template(ml)
            assert (pre, suf) == (([0], [2]) if which == "unigram" else ([2], [3]))
            docs = X.tokenize_passages([p for p, _ in text_pairs], ml)
            qrys = X.tokenize_queries([q for _, q in text_pairs], ml)
            idx = np.arange(len(text_pairs))
            ids, cu = pack_pairs_host(docs.tok, docs.off, qrys.tok, qrys.off, idx, idx, pre, suf,
                                      ml)
            bad = 0
            for i, (p, q) in enumerate(text_pairs):
                want = X.process_cross_encoder_document_and_query(p, q, ml).ids
                bad += list(want) != ids[cu[i]:cu[i + 1]].tolist()
            assert bad == 0, f"{bad} of {len(text_pairs)} pairs differ at max_length {ml}"
        # the batched protocol call is the per-pair one
        q = text_pairs[0][1]
        batch = X.process_cross_encoder_documents_and_query([p for p, _ in text_pairs[:5]], q, 40)
        assert [e.ids for e in batch] == [
            X.process_cross_encoder_document_and_query(p, q, 40).ids for p, _ in text_pairs[:5]]
        assert all(len(e.ids) <= 40 for e in batch)
    finally:
        X.tokenizer = saved


# ------------------------------------------------------------------ pack rule
@pytest.mark.parametrize("case", C.PACK_CASES, ids=[c[0] for c in C.PACK_CASES])
def test_pack_rule_hand_written(case):
    from improving_learned_index_amd.models import pack_pairs_host

    _, d, q, want = case
    dt, do = C.store(C.DOCS)
    qt, qo = C.store(C.QRYS)
    ids, cu = pack_pairs_host(dt, do, qt, qo, [d], [q], C.PREFIX, C.SUFFIX, C.MAX_LENGTH)
    assert ids.tolist() == want and cu.tolist() == [0, len(want)]
    assert ids.dtype == np.int32 and cu.dtype == np.int32


def test_pack_rule_batch_and_bad_index():
    from improving_learned_index_amd.models import pack_pairs_host

    dt, do = C.store(C.DOCS)
    qt, qo = C.store(C.QRYS)
    pd = [c[1] for c in C.PACK_CASES]
    pq = [c[2] for c in C.PACK_CASES]
    ids, cu = pack_pairs_host(dt, do, qt, qo, pd, pq, C.PREFIX, C.SUFFIX, C.MAX_LENGTH)
    assert ids.tolist() == [t for c in C.PACK_CASES for t in c[3]]
    assert cu.tolist() == np.cumsum([0] + [len(c[3]) for c in C.PACK_CASES]).tolist()
    with pytest.raises(IndexError):
        pack_pairs_host(dt, do, qt, qo, [len(C.DOCS)], [0], C.PREFIX, C.SUFFIX, C.MAX_LENGTH)
    with pytest.raises(IndexError):
        pack_pairs_host(dt, do, qt, qo, [0], [-1], C.PREFIX, C.SUFFIX, C.MAX_LENGTH)
