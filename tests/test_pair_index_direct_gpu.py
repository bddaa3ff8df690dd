"""The one-process route from a collection to the quantized index for the pairwise model
(index.run(pairwise=True, inverted_index_path=...), Indexer.build_index) against the text
route it leaves out (index --pairwise -> quantize -> inverted_index): the same three files
byte for byte, the same impact TSV, the same vocabulary and run file.  The seeded
encoder_xlmr_small encoder with the pair head of test_pairwise_entries_gpu.py over the
passages of test_pairwise_gpu.py, fp32 and bf16x3; and the BERT variant, also with maps
that are not in token order."""
import numpy as np
import pytest
import torch

import encoder_ref
from conftest import GOLDEN
from test_pairwise_entries_gpu import _pair_head, model_class, xlmr_checkpoint  # noqa: F401
from test_pairwise_gpu import PASSAGES

pytestmark = pytest.mark.gpu

FILES = ("vocab.txt", "inverted_index.idx", "inverted_index.dat")
# the one-term passage, repeated words and the punctuation line are among them
TEXTS = PASSAGES + ["water water water", "the sea, the earth; the world: hello (ok)"]
assert "single" in TEXTS and "ok ok ok world" in TEXTS


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from improving_learned_index_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible (GPU test run without a GPU)")
    tmp = tmp_path_factory.mktemp("pair_index_direct")
    sd, max_length = xlmr_checkpoint()
    ckpt = tmp / "DeepPairwiseImpact_latest.pt"
    torch.save({"model_state_dict": sd}, ckpt)
    coll = tmp / "collection.tsv"
    coll.write_text("".join(f"{i}\t{t}\n" for i, t in enumerate(TEXTS)), encoding="utf-8")
    return {"ckpt": ckpt, "coll": coll, "tmp": tmp, "max_length": max_length}


def _run(setup, precision, out, procs=1, **kw):
    from improving_learned_index_amd import index as index_cli

    n = index_cli.run(setup["coll"], "msmarco", out, str(setup["ckpt"]), num_processes=procs,
                      process_batch_size=7, tokenizer_path=GOLDEN / "tokenizer.json",
                      max_length=setup["max_length"], precision=precision, pairwise=True, **kw)
    assert n == len(TEXTS)


@pytest.fixture(scope="module")
def text_route(setup):
    """(precision, max_val) -> (impact TSV, index directory) of index --pairwise ->
    quantize_file -> InvertedIndexCreator, built once."""
    from improving_learned_index_amd.inverted_index import InvertedIndexCreator
    from improving_learned_index_amd.quantize import quantize_file

    cache = {}

    def get(precision, max_val=None):
        if (precision, max_val) not in cache:
            d = setup["tmp"] / f"text_{precision}_{max_val}"
            d.mkdir()
            tsv, q = d / "collection.index", d / "collection.quantized"
            if max_val is None:
                _run(setup, precision, tsv)
            else:
                tsv = get(precision)[0]
            quantize_file(tsv, q, max_val)
            InvertedIndexCreator(q, d / "index").run()
            cache[(precision, max_val)] = (tsv, d / "index", q)
        return cache[(precision, max_val)]
    return get


def _same_files(got, want):
    for f in FILES:
        assert (got / f).read_bytes() == (want / f).read_bytes(), f


def _entries(tsv):
    return [p.rsplit(": ", 1) for line in tsv.read_text(encoding="utf-8").splitlines()
            for p in (line.split(", ") if line else [])]


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_run_writes_the_text_routes_files(setup, text_route, precision, tmp_path,
                                          model_class):  # noqa: F811
    tsv, want, q = text_route(precision)
    # the collection exercises the route: pair postings survive, pairs were dropped
    vocab = (want / "vocab.txt").read_text(encoding="utf-8").splitlines()
    assert any("|" in t for t in vocab)
    T = [sum("|" not in k for k, _ in (p.rsplit(": ", 1) for p in line.split(", ")))
         for line in tsv.read_text(encoding="utf-8").splitlines()]
    assert sum("|" in k for k, _ in _entries(tsv)) < sum(t * (t - 1) // 2 for t in T)
    assert 1 in T
    _run(setup, precision, None, inverted_index_path=tmp_path / "a")
    _same_files(tmp_path / "a", want)
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == sorted(FILES)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["a"]
    # with the impact TSV as well: its bytes are the text route's
    _run(setup, precision, tmp_path / "b.index", inverted_index_path=tmp_path / "b")
    _same_files(tmp_path / "b", want)
    assert (tmp_path / "b.index").read_bytes() == tsv.read_bytes()


def test_run_with_tokenizer_workers(setup, text_route, tmp_path, model_class):  # noqa: F811
    """The worker pool's blobs (merged into device steps) give the same files and TSV."""
    tsv, want, _ = text_route("fp32")
    _run(setup, "fp32", tmp_path / "p.index", procs=2, inverted_index_path=tmp_path / "p")
    _same_files(tmp_path / "p", want)
    assert (tmp_path / "p.index").read_bytes() == tsv.read_bytes()


def test_run_max_val_is_quantizes_m(setup, text_route, tmp_path, model_class):  # noqa: F811
    top = max(float(v) for _, v in _entries(text_route("fp32")[0]))
    m = round(3.0 * top, 2)
    _, want, _ = text_route("fp32", m)
    _run(setup, "fp32", None, inverted_index_path=tmp_path / "m", max_val=m)
    _same_files(tmp_path / "m", want)
    assert (want / "inverted_index.dat").read_bytes() != \
        (text_route("fp32")[1] / "inverted_index.dat").read_bytes()  # other values


def test_steps_split_by_the_pair_budget(setup, text_route, tmp_path, monkeypatch,
                                        model_class):  # noqa: F811
    """A device step is cut where the sum of T^2 would pass di_encode_pairwise's limit:
    with a limit of 150 every batch of 7 passages takes several steps, same bytes."""
    from improving_learned_index_amd import indexer

    assert indexer._pair_step_ranges(np.array([0, 10, 12, 12, 22]), 150) == [(0, 3), (3, 4)]
    assert indexer._pair_step_ranges(np.array([0, 20, 22]), 150) == [(0, 1), (1, 2)]
    monkeypatch.setattr(indexer, "PAIR_STEP_T2", 150)
    tsv, want, _ = text_route("fp32")
    _run(setup, "fp32", tmp_path / "s.index", inverted_index_path=tmp_path / "s")
    _same_files(tmp_path / "s", want)
    assert (tmp_path / "s.index").read_bytes() == tsv.read_bytes()


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_build_index_in_memory_and_rank(setup, text_route, precision, tmp_path,
                                        model_class):  # noqa: F811
    from improving_learned_index_amd.indexer import Indexer
    from improving_learned_index_amd.inverted_index import InvertedIndex
    from improving_learned_index_amd.ranker import Ranker

    _, want_dir, q = text_route(precision)
    model = model_class.load(setup["ckpt"], tokenizer_path=GOLDEN / "tokenizer.json",
                             precision=precision, max_length=setup["max_length"])
    want = InvertedIndex(want_dir)
    indexer = Indexer(model, num_processes=1)
    whole = indexer.build_index(TEXTS, index_path=tmp_path / "ix")
    parts = indexer.build_index(iter([TEXTS[:5], TEXTS[5:6], TEXTS[6:]]))
    assert set(indexer.build_ms) == {"tokenize", "encode", "build"}
    _same_files(tmp_path / "ix", want_dir)
    terms = sorted(want.vocab)
    queries = [terms[i::max(1, len(terms) // 5)][:8] for i in range(6)]
    assert any("|" in t for qq in queries for t in qq)
    for got in (whole, parts):
        assert got.vocab == want.vocab
        assert got.score_batch(queries, 1000) == want.score_batch(queries, 1000)
    # queries made of two terms of one passage whose pair posting survived quantization
    picks = []
    for d, line in enumerate(q.read_text(encoding="utf-8").split("\n")):
        for k, v in (p.rsplit(": ", 1) for p in (line.split(", ") if line else [])):
            if "|" in k and int(v) > 0 and len(picks) < 4:
                picks.append(k)
                break
    assert picks
    (tmp_path / "q.tsv").write_text("".join(
        f"q{i}\t{' '.join(t.lstrip('▁') for t in k.split('|'))}\n" for i, k in enumerate(picks)),
        encoding="utf-8")
    runs = []
    for i, index_dir in enumerate((tmp_path / "ix", want_dir)):
        Ranker(index_dir, tmp_path / "q.tsv", tmp_path / f"run{i}.tsv", pairwise=True,
               tokenizer_path=GOLDEN / "tokenizer.json").run()
        runs.append((tmp_path / f"run{i}.tsv").read_bytes())
    assert runs[0] == runs[1] and runs[0]


def test_bert_variant_map_order(tmp_path, model_class):  # noqa: F811
    """variant "bert": absolute positions and the legacy counter's map, the model set up as
    in test_pairwise_entries_gpu.py.  The legacy maps come out in token order, so -- as
    there -- the same documents are also given with every map reversed: the step then
    permutes ids and term_tok into token order, and the TSV names go back through the
    permutation.  Files and TSV equal the text route's for both."""
    from improving_learned_index_amd.indexer import IndexBuild, Indexer
    from improving_learned_index_amd.inverted_index import InvertedIndexCreator
    from improving_learned_index_amd.quantize import quantize_file
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
    ids, cu, terms, tt, ct = model.pack_processed(proc)
    rev = np.concatenate([np.arange(ct[d + 1] - 1, ct[d] - 1, -1) for d in range(len(docs))])
    assert (np.diff(tt[rev][ct[0]:ct[1]]) < 0).all()

    def blob_of(order):
        enc = [terms[i].encode("utf-8") for i in order]
        off = np.zeros(len(enc) + 1, np.int64)
        off[1:] = np.cumsum([len(b) for b in enc])
        return ids, cu, b"".join(enc), off, tt[order], ct

    indexer = Indexer(model, num_processes=1)
    texts = {}
    for name, order in (("map", np.arange(len(terms))), ("rev", rev)):
        packed = blob_of(order)
        d = tmp_path / name
        d.mkdir()
        (d / "text.index").write_text(model.encode_packed_impacts(packed)(), encoding="utf-8")
        quantize_file(d / "text.index", d / "text.quantized")
        InvertedIndexCreator(d / "text.quantized", d / "want").run()
        build = IndexBuild(indexer, write_tsv=True)
        texts[name] = build._step(packed)
        build.inverted_index(None, d / "got")
        _same_files(d / "got", d / "want")
        assert texts[name] == (d / "text.index").read_text(encoding="utf-8")
        assert "|" in (d / "want" / "vocab.txt").read_text(encoding="utf-8")
    assert texts["map"] != texts["rev"]  # (the reversal changed the tie order)
    # and from the documents themselves, through Indexer.build_index
    with open(tmp_path / "direct.index", "w", encoding="utf-8") as f:
        indexer.build_index(docs, index_path=tmp_path / "got", file=f)
    _same_files(tmp_path / "got", tmp_path / "map" / "want")
    assert (tmp_path / "direct.index").read_text(encoding="utf-8") == texts["map"]


def test_refusals(setup, tmp_path, model_class):  # noqa: F811
    from improving_learned_index_amd.indexer import IndexBuild, Indexer

    model = model_class.load(setup["ckpt"], tokenizer_path=GOLDEN / "tokenizer.json",
                             precision="bf16", max_length=setup["max_length"])
    with pytest.raises(ValueError, match="fp32 or bf16x3"):
        IndexBuild(Indexer(model, num_processes=1))
    sd = {k: v for k, v in xlmr_checkpoint()[0].items() if "pairwise" not in k}
    torch.save({"model_state_dict": sd}, tmp_path / "single.pt")
    with pytest.raises(KeyError, match="pairwise_impact_score_encoder"):
        _run({**setup, "ckpt": tmp_path / "single.pt"}, "fp32", None,
             inverted_index_path=tmp_path / "x")
    assert not (tmp_path / "x").exists()
