"""The one-process route from a collection to the quantized index (index
--inverted_index_path, Indexer.build_index) against the text route it leaves out (index ->
quantize -> inverted_index -> InvertedIndex(path)): the same three files byte for byte,
the same impact TSV, the same search results.  Model and texts are set up as in
test_nano_beir_build_gpu.py (the golden encoder_xlmr_small fixture)."""
import json

import numpy as np
import pytest
import torch

import encoder_ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FILES = ("vocab.txt", "inverted_index.idx", "inverted_index.dat")


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from improving_learned_index_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible (GPU test run without a GPU)")
    tmp = tmp_path_factory.mktemp("index_direct")
    fx = json.loads((GOLDEN / "encoder_xlmr_small.json").read_text())
    sd = encoder_ref.seeded_state_dict(fx["state_dict_shapes"], fx["seed"], fx["std"])
    ckpt = tmp / "DeepImpact_latest.pt"
    torch.save({"model_state_dict": sd, "optimizer_state_dict": {}, "step": 0,
                "batch_size": 0}, ckpt)
    texts = [t for t in fx["texts"] if t.strip()]
    texts = texts + [" ".join(reversed(t.split())) for t in texts] + \
        [" ".join(t.split()[::2]) for t in texts if len(t.split()) > 3]
    coll = tmp / "collection.tsv"
    coll.write_text("".join(f"{i}\t{t}\n" for i, t in enumerate(texts)), encoding="utf-8")
    return {"fx": fx, "ckpt": ckpt, "texts": texts, "coll": coll, "tmp": tmp}


def _common(setup, precision, procs=1):
    return ["--collection_path", str(setup["coll"]), "--model_checkpoint_path",
            str(setup["ckpt"]), "--tokenizer_path", str(GOLDEN / "tokenizer.json"),
            "--max_length", str(setup["fx"]["max_length"]), "--precision", precision,
            "--process_batch_size", "4", "--num_processes", str(procs), "--device", "0"]


@pytest.fixture(scope="module")
def text_route(setup):
    """precision -> (impact TSV, index directory) of the three existing CLIs, built once."""
    from improving_learned_index_amd import index as index_cli
    from improving_learned_index_amd import quantize as quantize_cli
    from improving_learned_index_amd.inverted_index import InvertedIndexCreator

    cache = {}

    def get(precision, max_val=None):
        key = (precision, max_val)
        if key not in cache:
            d = setup["tmp"] / f"text_{precision}_{max_val}"
            d.mkdir()
            tsv, q = d / "collection.index", d / "collection.quantized"
            index_cli.main(_common(setup, precision) + ["--output_file_path", str(tsv)])
            quantize_cli.main(["-i", str(tsv), "-o", str(q)] +
                              (["-m", str(max_val)] if max_val is not None else []))
            InvertedIndexCreator(q, d / "index").run()
            assert (d / "index" / "inverted_index.dat").stat().st_size > 0
            cache[key] = (tsv, d / "index")
        return cache[key]
    return get


def _same_files(got, want):
    for f in FILES:
        assert (got / f).read_bytes() == (want / f).read_bytes(), f


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_cli_writes_the_text_routes_files(setup, text_route, precision, tmp_path):
    from improving_learned_index_amd import index as index_cli

    tsv, want = text_route(precision)
    index_cli.main(_common(setup, precision) + ["--inverted_index_path", str(tmp_path / "a")])
    _same_files(tmp_path / "a", want)
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == sorted(FILES)
    # with the impact TSV as well: its bytes are the text route's
    index_cli.main(_common(setup, precision) + ["--inverted_index_path", str(tmp_path / "b"),
                                                "--output_file_path", str(tmp_path / "b.index")])
    _same_files(tmp_path / "b", want)
    assert (tmp_path / "b.index").read_bytes() == tsv.read_bytes()


def test_cli_max_val_is_quantizes_m(setup, text_route, tmp_path):
    from improving_learned_index_amd import index as index_cli

    top = max(float(p.split(": ")[1]) for line in text_route("fp32")[0].read_text().splitlines()
              for p in line.split(", "))
    m = round(3.0 * top, 2)
    _, want = text_route("fp32", m)
    index_cli.main(_common(setup, "fp32") + ["--inverted_index_path", str(tmp_path / "m"),
                                             "--max_val", str(m)])
    _same_files(tmp_path / "m", want)
    assert (want / "inverted_index.dat").read_bytes() != \
        (text_route("fp32")[1] / "inverted_index.dat").read_bytes()  # other values


def test_cli_with_tokenizer_workers(setup, text_route, tmp_path):
    """The worker pool's blobs (merged into device steps) give the same files and TSV."""
    from improving_learned_index_amd import index as index_cli

    tsv, want = text_route("fp32")
    index_cli.main(_common(setup, "fp32", procs=2) + [
        "--inverted_index_path", str(tmp_path / "p"), "--output_file_path",
        str(tmp_path / "p.index")])
    _same_files(tmp_path / "p", want)
    assert (tmp_path / "p.index").read_bytes() == tsv.read_bytes()


def test_text_route_switch_gives_the_same_files(setup, text_route, tmp_path, monkeypatch):
    from improving_learned_index_amd import index as index_cli

    _, want = text_route("fp32")
    monkeypatch.setenv("DI_INDEX_TEXT_ROUTE", "1")
    index_cli.main(_common(setup, "fp32") + ["--inverted_index_path", str(tmp_path / "t")])
    _same_files(tmp_path / "t", want)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_build_index_in_memory_searches_like_the_files(setup, text_route, precision):
    from improving_learned_index_amd.encoder import EncoderConfig
    from improving_learned_index_amd.indexer import Indexer
    from improving_learned_index_amd.inverted_index import InvertedIndex
    from improving_learned_index_amd.models import DeepImpact

    fx = setup["fx"]
    cfg = EncoderConfig.from_hf({**fx["config"], "model_type": "xlm-roberta"})
    model = DeepImpact.load(setup["ckpt"], config=cfg, tokenizer_path=GOLDEN / "tokenizer.json",
                            precision=precision, max_length=fx["max_length"])
    want = InvertedIndex(text_route(precision)[1])
    texts = setup["texts"]
    indexer = Indexer(model, num_processes=1)
    whole = indexer.build_index(texts)
    parts = indexer.build_index(iter([texts[:5], texts[5:6], texts[6:]]))
    assert set(indexer.build_ms) == {"tokenize", "encode", "build"}
    terms = sorted(want.vocab)
    queries = [terms[i::max(1, len(terms) // 5)][:8] for i in range(6)] + [terms[:1], ["<none>"]]
    assert any(len(r) > 1 for r in want.score_batch(queries, 1000))
    for got in (whole, parts):
        assert got.vocab == want.vocab
        assert got.score_batch(queries, 1000) == want.score_batch(queries, 1000)
        assert got.score(queries[0], 3) == want.score(queries[0], 3)
        ids = [want.term_ids(q) for q in queries]
        (gd, gs, gn, _), (wd, ws, wn, _) = got.search_ids(ids, 10), want.search_ids(ids, 10)
        assert gn.tolist() == wn.tolist() and max(wn) == 10 and min(wn) == 0
        for i, n in enumerate(wn.tolist()):  # (the rows are filled up to their count)
            assert np.array_equal(gd[i, :n], wd[i, :n]) and np.array_equal(gs[i, :n], ws[i, :n])
        assert got.device_index.info() == want.device_index.info()


@pytest.mark.parametrize("extra, message", [
    (["--pairwise"], "does not take --pairwise"),
    (["--doc_range", "0:4"], "pass --device or --gpus 1"),
])
def test_refused_combinations(setup, tmp_path, capsys, extra, message):
    from improving_learned_index_amd import index as index_cli

    with pytest.raises(SystemExit) as ei:
        index_cli.main(_common(setup, "fp32") + ["--inverted_index_path", str(tmp_path / "x")]
                       + extra)
    assert ei.value.code == 2 and message in capsys.readouterr().err
    assert not (tmp_path / "x").exists()


def test_refused_with_more_than_one_rank(setup, tmp_path, capsys):
    from improving_learned_index_amd import index as index_cli

    args = [a for a in _common(setup, "fp32") if a not in ("--device", "0")]
    with pytest.raises(SystemExit) as ei:
        index_cli.main(args + ["--inverted_index_path", str(tmp_path / "x"), "--gpus", "2"])
    assert ei.value.code == 2 and "pass --device or --gpus 1" in capsys.readouterr().err
    with pytest.raises(SystemExit) as ei:  # neither output: argparse fails as before
        index_cli.main(args)
    assert ei.value.code == 2 and "--output_file_path" in capsys.readouterr().err
