"""The rerank CLI end to end on the GPU (small XLM-R fixture, seeded weights, the local
tokenizer, fp32): the device route -- impacts kept in a device store, candidates scored by
di_term_store_score and ordered by di_segment_order -- writes the bytes of the host route
(reranker.py:48-53,91 in Python), whatever the encode steps are."""
import json

import numpy as np
import pytest
import torch

import encoder_ref
import local_tokenizer
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

ML = 48


@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    """41 passages of 5 to 80 words (one longer than max_length) and 1001 short ones; four
    queries: two ordinary ones that share passages, one that shares no term with its
    candidates, one with 1001 candidates."""
    from improving_learned_index_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible (GPU test run without a GPU)")
    tmp = tmp_path_factory.mktemp("rerank")
    fx = json.loads((GOLDEN / "encoder_xlmr_small.json").read_text())
    sd = encoder_ref.seeded_state_dict(fx["state_dict_shapes"], fx["seed"], fx["std"])
    torch.save({"model_state_dict": sd}, tmp / "best.pt")
    local_tokenizer.save(tmp / "tokenizer.json")
    rng = np.random.default_rng(1)
    words = local_tokenizer.WORDS
    lens = [12, 30, 80, 5, 21, 9, 17, 26] * 5 + [14]
    passages = {str(100 + i): " ".join(rng.choice(words, n)) for i, n in enumerate(lens)}
    short = {str(5000 + i): " ".join(rng.choice(words[:40], 1 + i % 3)) for i in range(1001)}
    queries = {"9": "what is a learned sparse index", "4": "xylophone zeppelin",
               "11": "the water of a long day", "7": "neural ranking  model? the index"}
    long_ids = sorted(passages)
    cands = {"9": long_ids[:25], "4": long_ids[20:32], "11": list(short),
             "7": long_ids[10:41] + list(short)[:5]}
    (tmp / "collection.tsv").write_text(
        "".join(f"{p}\t{t}\n" for p, t in {**passages, **short}.items()), encoding="utf-8")
    (tmp / "queries.tsv").write_text("".join(f"{q}\t{t}\n" for q, t in queries.items()),
                                     encoding="utf-8")
    (tmp / "top.tsv").write_text(
        "".join(f"{q}\t{p}\t{r}\t{2000 - r}\n" for q in cands
                for r, p in enumerate(cands[q], start=1)), encoding="utf-8")
    return tmp, cands


def _args(tmp, out, *more):
    return ["--checkpoint_path", str(tmp / "best.pt"), "--tokenizer_path",
            str(tmp / "tokenizer.json"), "--top_k_run_file_path", str(tmp / "top.tsv"),
            "--queries_path", str(tmp / "queries.tsv"), "--collection_path",
            str(tmp / "collection.tsv"), "--max_length", str(ML), "--precision", "fp32",
            "--output_path", str(tmp / out), *more]


def test_device_route_writes_the_host_route_bytes(run_dir):
    from improving_learned_index_amd import reranker
    from improving_learned_index_amd.models import DeepImpact

    tmp, cands = run_dir
    saved = DeepImpact.tokenizer
    try:
        reranker.main(_args(tmp, "run.host.txt", "--score", "host"))
        reranker.main(_args(tmp, "run.device.txt", "--score", "device"))
        host = (tmp / "run.host.txt").read_bytes()
        assert (tmp / "run.device.txt").read_bytes() == host
        rows = [l.split("\t") for l in host.decode("utf-8").splitlines()]
        # every query in file order, 1001 candidates cut to 1000
        assert [len([r for r in rows if r[0] == q]) for q in cands] == [25, 12, 1000, 36]
        assert [r[0] for r in rows[:25]] == ["9"] * 25
        # the query that shares no term with its candidates: the int 0
        assert all(r[3] == "0" for r in rows if r[0] == "4")
        assert any(r[3] not in ("0", "0.0") for r in rows if r[0] == "11")

        # groups of one or two queries: the store grows between groups
        rr = reranker.ReRanker(tmp / "best.pt", tmp / "top.tsv", tmp / "queries.tsv",
                               tmp / "collection.tsv", tmp / "run.steps.txt",
                               tokenizer_path=tmp / "tokenizer.json", precision="fp32",
                               max_length=ML, score="auto", encode_batch=3)
        assert rr.score_route == "device"
        rr.run()
        assert (tmp / "run.steps.txt").read_bytes() == host
        # the device route really ran, and every passage was encoded once
        info = rr.store.info()
        assert info["n_docs"] == len({p for ps in cands.values() for p in ps}) == 41 + 1001
        assert info["n_terms"] > info["n_docs"] and not rr.cache
        assert rr.store.timing("ts_score")[1] >= 3 and rr.store.timing("ts_sort")[1] >= 3
        # rerank(qid, pids): a group of one, on a warm store
        got = rr.rerank("9", cands["9"])
        assert [f"9\t{p}\t{i}\t{s}" for i, (p, s) in enumerate(got, start=1)] == \
            ["\t".join(r) for r in rows[:25]]
        assert rr.store.info()["n_docs"] == info["n_docs"]
    finally:
        DeepImpact.tokenizer = saved


def test_forced_host_route(run_dir, monkeypatch):
    """DI_RERANK_HOST=1 takes the host route whatever --score says."""
    from improving_learned_index_amd import reranker
    from improving_learned_index_amd.models import DeepImpact

    tmp, _ = run_dir
    saved = DeepImpact.tokenizer
    monkeypatch.setenv("DI_RERANK_HOST", "1")
    try:
        rr = reranker.ReRanker(tmp / "best.pt", tmp / "top.tsv", tmp / "queries.tsv",
                               tmp / "collection.tsv", tmp / "unused.txt",
                               tokenizer_path=tmp / "tokenizer.json", precision="fp32",
                               max_length=ML, score="device")
        assert rr.score_route == "host"
        got = rr.rerank("4", ["100", "101"])
        assert got == [("100", 0), ("101", 0)] and rr.store is None and len(rr.cache) == 2
    finally:
        DeepImpact.tokenizer = saved
