"""The scorer's blocked device layout built on the GPU (di_index_create_device) against the
host route (di_index_create) and against the restatement of build_index() in
tests/index_layout_cases.py: the ten arrays byte for byte on every constructed case, from
host pointers and from device-resident postings; the same search results; the error paths;
and the Python routes on top (Indexer.build_index(layout=...), InvertedIndex(path) under
DI_INDEX_LAYOUT=device)."""
import ctypes
import json

import numpy as np
import pytest
import torch

import encoder_ref
import index_layout_cases as C
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FILES = ("vocab.txt", "inverted_index.idx", "inverted_index.dat")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from improving_learned_index_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible (GPU test run without a GPU)")


def _set_env(monkeypatch, env):
    for n in C.ENV_NAMES:
        monkeypatch.delenv(n, raising=False)
    for n, v in C.ENVS[env].items():
        monkeypatch.setenv(n, v)


def _create(case, layout, device_ptrs=False):
    from improving_learned_index_amd._lib import DeviceIndex

    if not device_ptrs:
        return DeviceIndex.from_postings(case.term_off, case.pdoc, case.pval, case.doc_lo,
                                         case.doc_hi, layout=layout)
    dev = torch.device("cuda", 0)
    off = torch.from_numpy(case.term_off).to(dev)
    doc = torch.from_numpy(np.resize(case.pdoc, max(case.pdoc.size, 1)).view(np.int32)).to(dev)
    val = torch.from_numpy(np.resize(case.pval, max(case.pval.size, 1))).to(dev)
    torch.cuda.synchronize()
    return DeviceIndex.from_postings(off, doc, val, case.doc_lo, case.doc_hi, layout="device")


def _assert_same_export(got, want, what):
    for k in C.ARRAYS:
        if want[k] is None:
            assert got[k] is None, (what, k)
            continue
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert got[k].tobytes() == want[k].tobytes(), (what, k)


@pytest.mark.parametrize("name, env", C.ALL)
def test_layout_bytes(name, env, monkeypatch):
    _set_env(monkeypatch, env)
    case = C.CASES[name]
    ref, _ = C.reference(name, env)
    host = _create(case, "host")
    h = host.export()
    _assert_same_export(h, ref, "host route vs restatement")
    assert host.layout() == {"n_ent": ref["n_ent"], "n_long": ref["n_long"],
                             "block_docs": ref["block_docs"], "has_flat": ref["has_flat"]}
    assert host.info() == {"n_terms": case.n_terms, "n_postings": ref["n_post"],
                           "n_docs": ref["n_docs"], "n_blocks": ref["nb"]}
    for ptrs in (False, True):
        dev = _create(case, "device", device_ptrs=ptrs)
        _assert_same_export(dev.export(), h, f"device route (device_ptrs={ptrs}) vs host route")
        assert dev.layout() == host.layout() and dev.info() == host.info()


def _same_search(a, b, q, cu, k=10):
    ra, rb = a.search_csr(q, cu, k, with_keys=True), b.search_csr(q, cu, k, with_keys=True)
    assert np.array_equal(ra[2], rb[2]) and ra[2].max() > 0
    for i, n in enumerate(ra[2].tolist()):
        for x, y in zip(ra, rb):
            if x.ndim == 2:
                assert np.array_equal(x[i, :n], y[i, :n])


@pytest.mark.parametrize("name", C.SEARCH_CASES)
def test_search_results_equal(name):
    case = C.CASES[name]
    q, cu = C.queries(case)
    host, dev = _create(case, "host"), _create(case, "device", device_ptrs=True)
    _same_search(host, dev, q, cu)
    _same_search(host, dev, q, cu, k=1000)
    if name != "d":
        return
    for setting in ("min_impact", "block_max", "packed"):
        host, dev = _create(case, "host"), _create(case, "device")
        for ix in (host, dev):
            if setting == "min_impact":
                ix.set_min_impact(16)        # reads seg
            elif setting == "block_max":
                ix.set_block_max(1.0)        # reads emax / wmax
            else:
                ix.set_packed(True)          # reads the layout through build_packed
        _same_search(host, dev, q, cu)


def _raw_create_device(term_off, pdoc, pval, doc_lo=0, doc_hi=0, flags=0):
    from improving_learned_index_amd import _lib

    h = ctypes.c_void_p()
    rc = _lib.lib().di_index_create_device(_lib.ptr(term_off), len(term_off) - 1, _lib.ptr(pdoc),
                                           _lib.ptr(pval), doc_lo, doc_hi, 0, None, flags,
                                           ctypes.byref(h))
    return rc, h


def test_non_monotone_device_term_off_is_einval():
    from improving_learned_index_amd import _lib

    dev = torch.device("cuda", 0)
    off = torch.tensor([0, 3, 2, 4], dtype=torch.int64, device=dev)
    doc = torch.arange(4, dtype=torch.int32, device=dev)
    val = torch.ones(4, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rc, h = _raw_create_device(off, doc, val, flags=_lib.DI_F_DEVICE_PTRS)
    assert rc == _lib.DI_EINVAL and not h.value
    assert "monotone" in _lib.lib().di_last_error().decode()
    off[0] = -1  # term_off[0] < 0
    off[2] = 3
    torch.cuda.synchronize()
    rc, h = _raw_create_device(off, doc, val, flags=_lib.DI_F_DEVICE_PTRS)
    assert rc == _lib.DI_EINVAL and not h.value
    # host pointers: the same status
    rc, h = _raw_create_device(np.array([0, 3, 2, 4], np.int64), np.arange(4, dtype=np.uint32),
                               np.ones(4, np.uint8))
    assert rc == _lib.DI_EINVAL and not h.value


def test_repeated_doc_overfilling_a_segment_is_einval():
    """The documented deviation: 2049 postings in one 2048-doc wave segment (a doc repeated
    inside a term) -- the host route takes it, the device route reports DI_EINVAL."""
    from improving_learned_index_amd import _lib

    docs = np.r_[np.arange(2048), 5].astype(np.uint32)
    off = np.array([0, docs.size], np.int64)
    val = np.full(docs.size, 3, np.uint8)
    rc, h = _raw_create_device(off, docs, val, doc_hi=32768)
    assert rc == _lib.DI_EINVAL and not h.value
    assert "2048" in _lib.lib().di_last_error().decode()
    # one posting fewer is fine, and equal to the host route
    case = C.Case("full_segment", [(docs[:2048], val[:2048])], doc_hi=32768)
    _assert_same_export(_create(case, "device").export(), _create(case, "host").export(),
                        "a full segment")


# ---------------------------------------------------------------------------------------
# end to end: the tiny model of test_index_direct_gpu.py
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from improving_learned_index_amd.encoder import EncoderConfig
    from improving_learned_index_amd.indexer import Indexer
    from improving_learned_index_amd.models import DeepImpact

    tmp = tmp_path_factory.mktemp("index_layout")
    fx = json.loads((GOLDEN / "encoder_xlmr_small.json").read_text())
    sd = encoder_ref.seeded_state_dict(fx["state_dict_shapes"], fx["seed"], fx["std"])
    ckpt = tmp / "DeepImpact_latest.pt"
    torch.save({"model_state_dict": sd, "optimizer_state_dict": {}, "step": 0,
                "batch_size": 0}, ckpt)
    texts = [t for t in fx["texts"] if t.strip()]
    texts = texts + [" ".join(reversed(t.split())) for t in texts]
    cfg = EncoderConfig.from_hf({**fx["config"], "model_type": "xlm-roberta"})
    model = DeepImpact.load(ckpt, config=cfg, tokenizer_path=GOLDEN / "tokenizer.json",
                            precision="fp32", max_length=fx["max_length"])
    return {"indexer": Indexer(model, num_processes=1), "texts": texts, "tmp": tmp}


def _queries_of(ix):
    terms = sorted(ix.vocab)
    return [terms[i::max(1, len(terms) // 5)][:8] for i in range(6)] + [terms[:1], ["<none>"]]


def test_build_index_layout_device_equals_host(tiny):
    indexer, texts, tmp = tiny["indexer"], tiny["texts"], tiny["tmp"]
    host = indexer.build_index(texts, index_path=tmp / "host", layout="host")
    dev = indexer.build_index(texts, index_path=tmp / "dev", layout="device")
    mem = indexer.build_index(texts, layout="device")     # the postings never visit the host
    for f in FILES:
        assert (tmp / "dev" / f).read_bytes() == (tmp / "host" / f).read_bytes(), f
    qs = _queries_of(host)
    assert any(len(r) > 1 for r in host.score_batch(qs, 1000))
    for got in (dev, mem):
        assert got.vocab == host.vocab
        _assert_same_export(got.device_index.export(), host.device_index.export(), "build_index")
        assert got.score_batch(qs, 1000) == host.score_batch(qs, 1000)
        assert got.device_index.info() == host.device_index.info()
    with pytest.raises(ValueError):
        indexer.build_index(texts, layout="gpu")


def test_inverted_index_from_files_under_the_switch(tiny, monkeypatch):
    from improving_learned_index_amd.inverted_index import InvertedIndex

    indexer, texts, tmp = tiny["indexer"], tiny["texts"], tiny["tmp"]
    if not (tmp / "files").exists():
        indexer.build_index(texts, index_path=tmp / "files")
    monkeypatch.setenv("DI_INDEX_LAYOUT", "host")
    host = InvertedIndex(tmp / "files")
    qs = _queries_of(host)
    for setting in ("device", None):                      # (the default is the device route)
        if setting is None:
            monkeypatch.delenv("DI_INDEX_LAYOUT")
        else:
            monkeypatch.setenv("DI_INDEX_LAYOUT", setting)
        dev = InvertedIndex(tmp / "files")
        _assert_same_export(dev.device_index.export(), host.device_index.export(),
                            "load_reference")
        assert dev.score_batch(qs, 1000) == host.score_batch(qs, 1000)


def test_timing_names_the_layout_kernels():
    from improving_learned_index_amd._lib import DeviceIndex

    case = C.CASES["c"]
    ix = DeviceIndex.from_postings(case.term_off, case.pdoc, case.pval, case.doc_lo, case.doc_hi,
                                   layout="device", timing=True)
    for name in ("il_check", "il_input", "il_count", "il_scan", "il_compact", "il_hist",
                 "il_scatter", "il_heads", "il_entries", "il_long", "il_segment", "il_deal"):
        ms, launches = ix.timing(name)
        assert launches >= 1 and ms >= 0.0, name
