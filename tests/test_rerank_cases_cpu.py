"""CPU checks that the cases of tests/rerank_cases.py can tell a right device scorer from
a wrong one (the add order, the int 0 of a candidate without a match, ties and the cut at
1000), and the route selection of reranker.ReRanker with a model that has no HIP encoder."""
import random

import numpy as np
import pytest

import rerank_cases as R
from conftest import GOLDEN


def _changed_by_reverse_order(value_lists):
    vs = [v for v in value_lists if len(v) >= 3]
    return sum(R.sum_bits(v) != R.sum_bits(v, reverse=True) for v in vs), len(vs)


def test_reverse_add_order_changes_the_bits():
    """The recipe's values: over 2000 draws of 3 to 8 terms, and over the candidates of the
    two cases with at least 3 matches, summing in reverse query order changes the float32
    bits of at least 20% (44% measured over the draws)."""
    rng = np.random.default_rng(0)
    changed, n = _changed_by_reverse_order(
        [R.draw_impacts(rng, int(rng.integers(3, 9))) for _ in range(2000)])
    print("draws:", changed, "of", n)
    assert n == 2000 and changed >= 0.2 * n
    for case in (R.abi_case(), R.ranking_case()):
        passages, queries, cands, _ = case
        changed, n = _changed_by_reverse_order(
            [R.matched_values(passages, q, c) for q, cs in zip(queries, cands) for c in cs])
        print("case:", changed, "of", n)
        assert n >= 50 and changed >= 0.2 * n


def test_abi_case_covers_what_it_says():
    passages, queries, cands, ref = R.abi_case()
    assert sorted(len(p) for p in passages) == sorted(2 * list(R.PASSAGE_SIZES))
    assert [len(q) for q in queries[:-1]] == list(R.QUERY_SIZES) and cands[-1] == []
    # ids arrive unsorted, one passage descending (the sort has work to do either way)
    ids = [t for t, _ in passages[9]]
    assert ids == sorted(ids, reverse=True) and ids != sorted(ids)
    ids = [t for t, _ in passages[20]]
    assert ids != sorted(ids) and ids != sorted(ids, reverse=True)
    held = {t for p in passages for t, _ in p}
    for q in queries[2:-1]:
        assert any(t not in held for t in q) and len(set(q)) < len(q)
    assert cands[2].count(5) == 3
    # matched and unmatched candidates, zero sums of both kinds
    match = np.concatenate([m for _, _, m in ref])
    assert (match == 0).any() and (match >= 3).sum() >= 50
    # a repeated id adds twice
    q, c = queries[3], 10
    d = dict(passages[c])
    assert q.count(q[1]) >= 2 and q[1] in d


def test_ranking_case_has_unmatched_candidates_ties_and_a_cut():
    passages, queries, cands, ref = R.ranking_case()
    for q, cs, (scores, bits, match) in zip(queries, cands, ref):
        assert len(cs) == R.CUT + 1
        assert (match == 0).any()  # the int 0
        zero_matched = [s for s, m in zip(scores, match) if m > 0 and s == 0]
        assert zero_matched and all(isinstance(s, np.float32) for s in zero_matched)
        ranked = sorted(scores, reverse=True)
        ties = [r for r in range(R.CUT) if ranked[r] == ranked[r + 1]]
        assert len(ties) >= 2 and ties[-1] == R.CUT - 1  # inside the list, across rank 1000
        # the planted order matters: ordering by pid alone is a different answer
        want = R.reference_ranking(cs, scores)
        assert len(want) == R.CUT
        assert [p for p, _ in want] != sorted(cs)[:R.CUT]
        assert [p for p, _ in want] != sorted(cs, reverse=True)[:R.CUT]
        # ties keep the candidates' input order
        by_score = {}
        for p, s in want:
            by_score.setdefault(float(s), []).append(p)
        assert any(len(v) > 1 for v in by_score.values())
        assert all(v == sorted(v) for v in by_score.values())


# ------------------------------------------------------------------ route selection
class _FakeModel:
    """Deterministic term impacts per passage (np.float32); no HIP encoder."""

    def get_impact_scores_batch(self, docs):
        from improving_learned_index_amd import models

        out = []
        for d, (_, tmap) in zip(docs, models.DeepImpact.process_documents(docs)):
            rng = random.Random(d)
            out.append([(t, np.float32(rng.uniform(-1, 5))) for t in tmap])
        return out


@pytest.fixture()
def small_run(tmp_path):
    from improving_learned_index_amd import models

    models.DeepImpact.set_tokenizer(GOLDEN / "tokenizer.json")
    rng = random.Random(8)
    words = [f"w{i}" for i in range(30)]
    coll = {str(p): " ".join(rng.choice(words) for _ in range(rng.randint(1, 10)))
            for p in range(80)}
    (tmp_path / "coll.tsv").write_text("".join(f"{p}\t{t}\n" for p, t in coll.items()))
    queries = {str(q): " ".join(rng.choice(words) for _ in range(rng.randint(1, 4)))
               for q in range(6)}
    queries["6"] = "zz9 qq8"  # shares no term with any passage: every score is the int 0
    (tmp_path / "q.tsv").write_text("".join(f"{q}\t{t}\n" for q, t in queries.items()))
    lines = []
    for q in queries:
        pids = rng.sample(sorted(coll), 30)
        lines += [f"{q}\t{p}\t{r}\t{100 - r}\n" for r, p in enumerate(pids, start=1)]
    (tmp_path / "topk.tsv").write_text("".join(lines))
    return tmp_path, coll, queries


def test_device_route_needs_a_device_encoder(small_run):
    from improving_learned_index_amd import reranker

    tmp, _, _ = small_run
    args = (None, tmp / "topk.tsv", tmp / "q.tsv", tmp / "coll.tsv", tmp / "out.tsv")
    with pytest.raises(ValueError):
        reranker.ReRanker(*args, model=_FakeModel(), score="device")
    with pytest.raises(ValueError):
        reranker.ReRanker(*args, model=_FakeModel(), score="gpu")


def test_auto_without_a_device_encoder_is_the_host_route(small_run):
    """score='auto' (the default) with the fake model: the host route, whose bytes are the
    restatement's -- reranker.py:52-53,91 through RunFile.writelines."""
    from improving_learned_index_amd import models, reranker

    tmp, coll, queries = small_run
    fake = _FakeModel()
    rr = reranker.ReRanker(None, tmp / "topk.tsv", tmp / "q.tsv", tmp / "coll.tsv",
                           tmp / "out.tsv", batch_size=7, model=fake)
    assert rr.score_route == "host" and rr.store is None
    rr.run()
    lines = []
    for qid, pids in rr.top_k:
        terms = models.DeepImpact.process_query(queries[qid])
        scores = [R.reference_score(dict(fake.get_impact_scores_batch([coll[p]])[0]), terms)
                  for p in pids]
        for rank, (pid, score) in enumerate(R.reference_ranking(pids, scores), start=1):
            lines.append(f"{qid}\t{pid}\t{rank}\t{score}\n")
    got = (tmp / "out.tsv").read_bytes()
    assert got == "".join(lines).encode("utf-8")
    assert b"\t0\n" in got and len(rr.cache) == len({p for _, ps in rr.top_k for p in ps})
    # the same bytes with the route named
    rh = reranker.ReRanker(None, tmp / "topk.tsv", tmp / "q.tsv", tmp / "coll.tsv",
                           tmp / "out.host.tsv", model=fake, score="host", encode_batch=3)
    rh.run()
    assert (tmp / "out.host.tsv").read_bytes() == got
