"""SparseSearch's two build routes on the GPU (nano_beir.py): the float index assembled on
the device from the encoder's device output (build="device") gives exactly the search
results of the reference's host route (build="host") -- the dicts, their iteration order
and the floats -- and, in fp32, the metrics of the oracle chain of test_nano_beir_gpu.py.
Model and texts are set up as there (the golden encoder_xlmr_small fixture)."""
import json

import numpy as np
import pytest
import torch

import encoder_ref
import oracle
from conftest import GOLDEN
from test_nano_beir_gpu import _dataset

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from improving_learned_index_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible (GPU test run without a GPU)")
    tmp = tmp_path_factory.mktemp("nano_build")
    fx = json.loads((GOLDEN / "encoder_xlmr_small.json").read_text())
    sd = encoder_ref.seeded_state_dict(fx["state_dict_shapes"], fx["seed"], fx["std"])
    ckpt = tmp / "ckpt.pt"
    torch.save({"model_state_dict": sd, "optimizer_state_dict": {}, "step": 0,
                "batch_size": 0}, ckpt)
    texts = [t for t in fx["texts"] if t.strip()]
    texts = texts + [" ".join(reversed(t.split())) for t in texts] + \
        [" ".join(t.split()[::2]) for t in texts if len(t.split()) > 3]
    docs, queries, qrels = _dataset(tmp, texts)
    return {"fx": fx, "sd": sd, "ckpt": ckpt, "corpus": dict(docs), "queries": queries,
            "qrels": qrels, "docs": docs}


def _model(setup, precision):
    from improving_learned_index_amd.encoder import EncoderConfig
    from improving_learned_index_amd.models import DeepImpact

    fx = setup["fx"]
    cfg = EncoderConfig.from_hf({**fx["config"], "model_type": "xlm-roberta"})
    return DeepImpact.load(setup["ckpt"], config=cfg, tokenizer_path=GOLDEN / "tokenizer.json",
                           precision=precision, max_length=fx["max_length"])


def _identical(a, b):
    assert list(a) == list(b)
    for q in a:
        assert list(a[q].items()) == list(b[q].items()), q


@pytest.fixture(scope="module")
def results(setup):
    """precision -> (device-route SparseSearch, its results, host-route SparseSearch, its
    results), computed once."""
    from improving_learned_index_amd.nano_beir import SparseSearch

    cache = {}

    def get(precision):
        if precision not in cache:
            model = _model(setup, precision)
            assert len(setup["corpus"]) > 2 * 7  # three appends at encode_batch=7
            dev = SparseSearch(model, 16, build="device", encode_batch=7)
            host = SparseSearch(model, 16, build="host")
            cache[precision] = (dev, dev.search(setup["queries"], setup["corpus"], 1000),
                                host, host.search(setup["queries"], setup["corpus"], 1000))
        return cache[precision]
    return get


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_device_build_equals_host_build(setup, results, precision):
    dev, got, host, want = results(precision)
    assert dev.build_route == "device" and host.build_route == "host"
    _identical(got, want)
    assert any(len(r) > 1 for r in got.values())
    assert set(dev.vocab) == set(host.vocab)
    # the same bytes on the device, under the routes' term numbering
    d_start, d_off, d_doc, d_imp = dev.inverted_index.export()
    h_start, h_off, h_doc, h_imp = host.inverted_index.export()
    assert d_doc.size == h_doc.size
    for t, i in host.vocab.items():
        j = dev.vocab[t]
        assert d_off[j].tolist() == h_off[i].tolist(), t
        n = int(h_off[i, -1])
        a, b = int(h_start[i]), int(d_start[j])
        assert d_doc[b:b + n].tobytes() == h_doc[a:a + n].tobytes(), t
        assert d_imp[b:b + n].tobytes() == h_imp[a:a + n].tobytes(), t
    # a term that kept no posting is in neither vocabulary
    count = d_off[:, -1]
    assert all(count[j] > 0 for j in dev.vocab.values())
    assert set(dev.build_ms) == {"tokenize", "encode", "build"}


def test_device_build_matches_oracle_chain(setup, results):
    from improving_learned_index_amd.metrics import evaluate_retrieval
    from improving_learned_index_amd.models import DeepImpact

    _, got, _, _ = results("fp32")
    fx, sd, docs, queries, qrels = (setup[k] for k in ("fx", "sd", "docs", "queries", "qrels"))
    proc = [DeepImpact.process_document(t, fx["max_length"]) for _, t in docs]
    S = max(len(e.ids) for e, _ in proc)
    ids = np.ones((len(proc), S), np.int64)
    mask = np.zeros_like(ids)
    for i, (e, _) in enumerate(proc):
        ids[i, :len(e.ids)] = e.ids
        mask[i, :len(e.ids)] = 1
    with torch.no_grad():
        tok = encoder_ref.forward(sd, fx["config"], torch.from_numpy(ids),
                                  torch.from_numpy(mask), "xlmr", "softplus").numpy()
    term_imps = [[(t, np.float32(tok[i, j])) for t, j in m.items()]
                 for i, (_, m) in enumerate(proc)]
    ora = oracle.SparseIndex([d for d, _ in docs], term_imps)
    qids = list(queries)
    res = ora.search([list(DeepImpact.process_query(queries[q])) for q in qids], 1000)
    want = {q: {d: float(s) for d, s in r} for q, r in zip(qids, res)}
    assert evaluate_retrieval(qrels, got, (10, 100, 1000)) == \
        evaluate_retrieval(qrels, want, (10, 100, 1000))
    assert list(got) == list(want)


def test_auto_env_and_evaluator_routes(setup, results, monkeypatch):
    from improving_learned_index_amd.nano_beir import NanoBEIREvaluator, SparseSearch

    dev, got, _, _ = results("fp32")
    monkeypatch.setenv("DI_SPARSE_HOST_BUILD", "1")
    forced = SparseSearch(dev.model, 16, build="device")
    assert forced.build_route == "host"
    _identical(forced.search(setup["queries"], setup["corpus"], 1000), got)
    monkeypatch.delenv("DI_SPARSE_HOST_BUILD")
    ev = NanoBEIREvaluator(batch_size=16, build="device", encode_batch=5)
    res, qrels = ev.search(dev.model, (setup["corpus"], setup["queries"], setup["qrels"]))
    _identical(res, got)
    with pytest.raises(ValueError):
        SparseSearch(dev.model, 16, build="gpu")


def test_device_build_needs_a_device_encoder():
    from improving_learned_index_amd.nano_beir import SparseSearch

    class FakeModel:
        def get_impact_scores_batch(self, texts):
            return [[(w, np.float32(1.0)) for w in t.split()] for t in texts]

        def process_query(self, q):
            return q.split()

    with pytest.raises(ValueError):
        SparseSearch(FakeModel(), 16, build="device")
    ss = SparseSearch(FakeModel(), 16)  # auto: the host route, as before
    assert ss.build_route == "host"
    assert list(ss.search({"q": "b"}, {"x": "a b", "y": "b c"}, 10)["q"]) == ["x", "y"]
