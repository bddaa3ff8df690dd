"""GPU checks of the cross-encoder path (csrc/cross.hip): di_pairs_pack against the numpy
pack rule, di_encode_pairs against the existing encode (bit for bit) and against the
plain PyTorch fp32 oracle at token 0 (the reference's last_hidden_state[:, 0, :],
src/deep_impact/models/cross_encoder.py:22-23), di_segment_order against Python's sorted
(src/deep_impact/evaluation/cross_encoder_reranker.py:62), and the CLI end to end: the
device-assembled route, the joined-string route and a restatement of
cross_encoder_reranker.py:41-62 write the same bytes.
Tolerance against the fp32 oracle: the project's fp32-parity bound rtol 1e-3, atol 1e-6.
"""
import contextlib
import json

import numpy as np
import pytest
import torch

import cross_cases as C
import encoder_ref
import local_tokenizer
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

VOCAB = 1024
ML = 512


@pytest.fixture(scope="module")
def L():
    from improving_learned_index_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible (GPU test run without a GPU)")
    return _lib


@pytest.fixture(scope="module")
def base_fx():
    return json.loads((GOLDEN / "encoder_xlmr_base.json").read_text())


@pytest.fixture(scope="module")
def small(base_fx):
    """hidden 768, 12 heads, 2 layers, vocabulary 1024: seeded weights and config."""
    shapes = []
    for k, shape, dt in base_fx["state_dict_shapes"]:
        if "encoder.layer." in k and int(k.split("encoder.layer.")[1].split(".")[0]) >= 2:
            continue
        if k.endswith("word_embeddings.weight"):
            shape = [VOCAB, shape[1]]
        shapes.append((k, shape, dt))
    sd = encoder_ref.seeded_state_dict(shapes, 23, 0.02)
    cfg = dict(base_fx["config"], vocab_size=VOCAB, num_hidden_layers=2)
    return sd, cfg


def _cfg(E, c, act):
    return E.EncoderConfig(variant="xlmr", activation=act, vocab_size=c["vocab_size"],
                           hidden=c["hidden_size"], layers=c["num_hidden_layers"],
                           heads=c["num_attention_heads"], intermediate=c["intermediate_size"],
                           max_positions=c["max_position_embeddings"],
                           type_vocab=c["type_vocab_size"], pad_id=c["pad_token_id"],
                           layer_norm_eps=c["layer_norm_eps"])


@pytest.fixture(scope="module")
def encoders(L, small):
    """One encoder per (precision, head), made on first use."""
    from improving_learned_index_amd import encoder as E

    sd, cfg = small
    made = {}

    def get(precision, act="softplus"):
        if (precision, act) not in made:
            made[precision, act] = E.DeviceEncoder(sd, _cfg(E, cfg, act), precision=precision)
        return made[precision, act]

    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def edge_batch():
    """Stores and pairs whose sequences (max_length 512, one prefix and one suffix id) come
    out at 2, 3, 16, 17, 256, 257, 384, 385 and 512 tokens, a 700-token passage cut to 512,
    the cut inside a query and at the passage / query boundary, a passage used by several
    pairs and a query used by several pairs."""
    rng = np.random.default_rng(3)
    doc_lens = [0, 1, 10, 11, 250, 251, 380, 381, 500, 700, 510, 505]
    qry_lens = [0, 4, 10, 2, 30]
    docs = [rng.integers(5, VOCAB, n).tolist() for n in doc_lens]
    qrys = [rng.integers(5, VOCAB, n).tolist() for n in qry_lens]
    #        2       3       16      17      256     257     384     385     512
    pairs = [(0, 0), (1, 0), (2, 1), (3, 1), (4, 1), (5, 1), (6, 3), (7, 3), (8, 2),
             (9, 1),            # 700-token passage: the cut inside the passage
             (10, 1),           # 510 + 4: the cut at the passage / query boundary
             (11, 4),           # 505 + 30: the cut inside the query
             (4, 2), (4, 4),    # a passage used by several pairs
             (2, 1), (6, 1)]    # a query used by several pairs
    want_lens = [2, 3, 16, 17, 256, 257, 384, 385, 512, 512, 512, 512, 262, 282, 16, 386]
    dt, do = C.store(docs)
    qt, qo = C.store(qrys)
    pd = np.array([p[0] for p in pairs], np.int32)
    pq = np.array([p[1] for p in pairs], np.int32)
    return dt, do, qt, qo, pd, pq, want_lens


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


# ------------------------------------------------------------------ di_pairs_pack
@pytest.mark.parametrize("ptrs", ["host", "device"])
def test_pairs_pack_equals_numpy_packer(L, edge_batch, ptrs):
    from improving_learned_index_amd.models import pack_pairs_host

    def run(dt, do, qt, qo, pd, pq, fmt):
        if ptrs == "host":
            ids, cu, nt, ml = L.pairs_pack(dt, do, qt, qo, pd, pq, fmt)
            return ids, cu, nt, ml
        # (an empty store still needs a valid device address)
        args = _dev(dt if dt.size else np.zeros(1, np.int32), do,
                    qt if qt.size else np.zeros(1, np.int32), qo, pd, pq)
        ids, cu, nt, ml = L.pairs_pack(*args, fmt)
        torch.cuda.synchronize()
        return ids.cpu().numpy(), cu.cpu().numpy(), nt, ml

    # the hand-written cases of tests/test_cross_cpu.py, one call
    dt, do = C.store(C.DOCS)
    qt, qo = C.store(C.QRYS)
    pd = np.array([c[1] for c in C.PACK_CASES], np.int32)
    pq = np.array([c[2] for c in C.PACK_CASES], np.int32)
    ids, cu, nt, ml = run(dt, do, qt, qo, pd, pq, L.pair_format(C.PREFIX, C.SUFFIX, C.MAX_LENGTH))
    assert ids.tolist() == [t for c in C.PACK_CASES for t in c[3]]
    assert cu.tolist() == np.cumsum([0] + [len(c[3]) for c in C.PACK_CASES]).tolist()
    assert (nt, ml) == (int(cu[-1]), 16)

    # the length edges, a truncated 700-token passage, shared passages and queries
    dt, do, qt, qo, pd, pq, want_lens = edge_batch
    ids, cu, nt, ml = run(dt, do, qt, qo, pd, pq, L.pair_format([0], [2], ML))
    w_ids, w_cu = pack_pairs_host(dt, do, qt, qo, pd, pq, [0], [2], ML)
    assert np.diff(w_cu).tolist() == want_lens
    assert np.array_equal(cu, w_cu) and np.array_equal(ids, w_ids)
    assert (nt, ml) == (int(w_cu[-1]), 512)

    # two prefix ids, no suffix; more pairs than one scan chunk (1024) with a carry
    rng = np.random.default_rng(9)
    pd2 = rng.integers(0, len(do) - 1, 2500).astype(np.int32)
    pq2 = rng.integers(0, len(qo) - 1, 2500).astype(np.int32)
    ids, cu, nt, ml = run(dt, do, qt, qo, pd2, pq2, L.pair_format([7, 8], [], 40))
    w_ids, w_cu = pack_pairs_host(dt, do, qt, qo, pd2, pq2, [7, 8], [], 40)
    assert np.array_equal(cu, w_cu) and np.array_equal(ids, w_ids)

    # no pairs
    ids, cu, nt, ml = run(dt, do, qt, qo, pd[:0], pq[:0], L.pair_format([0], [2], ML))
    assert (ids.size, cu.tolist(), nt, ml) == (0, [0], 0, 0)


@pytest.mark.parametrize("ptrs", ["host", "device"])
@pytest.mark.parametrize("bad", [(12, 0), (-1, 0), (0, 5), (0, -3)])
def test_pairs_pack_bad_index_is_einval(L, edge_batch, ptrs, bad):
    dt, do, qt, qo, pd, pq, _ = edge_batch
    pd, pq = pd.copy(), pq.copy()
    pd[3], pq[3] = pd[3] if bad[0] == 0 else bad[0], pq[3] if bad[1] == 0 else bad[1]
    args = (dt, do, qt, qo, pd, pq) if ptrs == "host" else _dev(dt, do, qt, qo, pd, pq)
    with pytest.raises(L.DIError) as ei:
        L.pairs_pack(*args, L.pair_format([0], [2], ML))
    assert ei.value.code == -1  # DI_EINVAL


# ------------------------------------------------------------------ di_encode_pairs
@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
def test_encode_pairs_bitexact_with_existing_encode(L, encoders, edge_batch, precision):
    """The same arithmetic as encode_packed over the host-packed batch with token 0 of each
    sequence as its only term: this checks the wiring (and the timing names)."""
    from improving_learned_index_amd.models import pack_pairs_host

    enc = encoders(precision)
    dt, do, qt, qo, pd, pq, _ = edge_batch
    fmt = L.pair_format([0], [2], ML)
    ids, cu = pack_pairs_host(dt, do, qt, qo, pd, pq, [0], [2], ML)
    n = len(pd)
    want = enc.encode_packed(ids, cu, np.zeros(n, np.int32), np.arange(n + 1, dtype=np.int32))
    enc.timing("pairs_scan", reset=True)
    got = enc.encode_pairs(dt, do, qt, qo, pd, pq, fmt, timing=True)
    assert got.dtype == np.float32 and got.shape == (n,)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert enc.timing("pairs_scan")[1] == 1 and enc.timing("pairs_copy")[1] == 1
    # device pointers, a smaller batch after a larger one (the workspace keeps its size)
    d = _dev(dt, do, qt, qo, pd[2:9], pq[2:9])
    got_d = enc.encode_pairs(*d, fmt)
    torch.cuda.synchronize()
    assert np.array_equal(got_d.cpu().numpy().view(np.uint32), want[2:9].view(np.uint32))
    # a bad pair index: DI_EINVAL, and the encoder still works afterwards
    with pytest.raises(L.DIError) as ei:
        enc.encode_pairs(dt, do, qt, qo, np.array([0, 99], np.int32), np.array([0, 0], np.int32),
                         fmt)
    assert ei.value.code == -1
    again = enc.encode_pairs(dt, do, qt, qo, pd[:4], pq[:4], fmt)
    assert np.array_equal(again.view(np.uint32), want[:4].view(np.uint32))


@contextlib.contextmanager
def _one_torch_thread():
    """The CPU oracle on one thread: a torch thread pool started in this process would
    deadlock the workers that tests/test_distributed_cpu.py forks from it later."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def _oracle_cls(sd, cfg, ids, cu, act):
    lens = np.diff(cu)
    pad = np.ones((len(lens), int(lens.max())), np.int64)
    mask = np.zeros_like(pad)
    for i, n in enumerate(lens):
        pad[i, :n] = ids[cu[i]:cu[i + 1]]
        mask[i, :n] = 1
    with torch.no_grad(), _one_torch_thread():
        return encoder_ref.forward(sd, cfg, torch.from_numpy(pad), torch.from_numpy(mask), "xlmr",
                                   act).numpy()[:, 0]


ORACLE_ML = 128
# sequences of 2, 3, 17, 42 and 22 tokens and a 250-token passage cut to 128
ORACLE_PAIRS = [(0, 0), (1, 0), (3, 1), (2, 4), (2, 2), (4, 1)]


@pytest.fixture(scope="module")
def oracle_scores(small, edge_batch):
    """Token-0 impacts of the fp32 oracle on six sequences of the edge stores at max_length
    128, per head (computed once; the length edges up to 512 are checked bit for bit
    against the existing encode above)."""
    from improving_learned_index_amd.models import pack_pairs_host

    sd, cfg = small
    dt, do, qt, qo, _, _, _ = edge_batch
    pd = np.array([p[0] for p in ORACLE_PAIRS], np.int32)
    pq = np.array([p[1] for p in ORACLE_PAIRS], np.int32)
    ids, cu = pack_pairs_host(dt, do, qt, qo, pd, pq, [0], [2], ORACLE_ML)
    assert np.diff(cu).tolist() == [2, 3, 17, 42, 22, 128]
    return pd, pq, {act: _oracle_cls(sd, cfg, ids, cu, act) for act in ("softplus", "relu")}


@pytest.mark.parametrize("act", ["softplus", "relu"])
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_encode_pairs_matches_oracle(L, encoders, edge_batch, oracle_scores, precision, act):
    enc = encoders(precision, act)
    dt, do, qt, qo, _, _, _ = edge_batch
    pd, pq, want = oracle_scores
    got = enc.encode_pairs(dt, do, qt, qo, pd, pq, L.pair_format([0], [2], ORACLE_ML))
    print(precision, act, "got", got.tolist(), "want", want[act].tolist())
    np.testing.assert_allclose(got, want[act], rtol=1e-3, atol=1e-6)


def test_encode_pairs_matches_oracle_xlmr_base_shape(L, base_fx):
    """The 12-layer xlm-roberta-base shape, bf16x3 (the CLI's default precision)."""
    from improving_learned_index_amd import encoder as E
    from improving_learned_index_amd.models import pack_pairs_host

    sd = encoder_ref.seeded_state_dict(base_fx["state_dict_shapes"], base_fx["seed"],
                                       base_fx["std"])
    rng = np.random.default_rng(5)
    docs = [rng.integers(5, 250002, n).tolist() for n in (30, 3, 70, 17)]
    qrys = [rng.integers(5, 250002, n).tolist() for n in (6, 9)]
    dt, do = C.store(docs)
    qt, qo = C.store(qrys)
    pd = np.array([0, 1, 2, 3], np.int32)
    pq = np.array([0, 1, 0, 1], np.int32)
    ids, cu = pack_pairs_host(dt, do, qt, qo, pd, pq, [0], [2], 48)
    want = _oracle_cls(sd, base_fx["config"], ids, cu, "softplus")
    enc = E.DeviceEncoder(sd, _cfg(E, base_fx["config"], "softplus"), precision="bf16x3")
    try:
        got = enc.encode_pairs(dt, do, qt, qo, pd, pq, L.pair_format([0], [2], 48))
    finally:
        enc.close()
    np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-6)


# ------------------------------------------------------------------ di_segment_order
def _sorted_positions(scores, cu):
    out = []
    for a, b in zip(cu[:-1], cu[1:]):
        seg = scores[a:b].tolist()
        out += [p for p, _ in sorted(zip(range(len(seg)), seg), key=lambda x: x[1],
                                     reverse=True)]
    return out


@pytest.mark.parametrize("ptrs", ["host", "device"])
def test_segment_order_equals_python_sorted(L, ptrs):
    rng = np.random.default_rng(17)
    lens = [0, 1, 2, 63, 64, 65, 1000, 4096, 0]
    cu = np.cumsum([0] + lens).astype(np.int32)
    # many exact ties (ReLU zeros, a few repeated values), -0.0 beside +0.0, negatives, inf
    pool = np.array([0.0, 0.0, 0.0, -0.0, 1.5, 1.5, -2.25, np.inf, -np.inf, 3e-39, -3e-39,
                     1e30, 0.1], np.float32)
    scores = np.where(rng.random(cu[-1]) < 0.6, rng.choice(pool, cu[-1]),
                      rng.standard_normal(cu[-1]).astype(np.float32)).astype(np.float32)
    scores[cu[3]:cu[3] + 4] = [-0.0, 0.0, -0.0, 0.0]
    want = _sorted_positions(scores, cu)
    if ptrs == "host":
        got = L.segment_order(scores, cu)
    else:
        s, c = _dev(scores, cu)
        got = L.segment_order(s, c).cpu().numpy()
    assert got.tolist() == want


@pytest.mark.parametrize("ptrs", ["host", "device"])
def test_segment_order_longer_segment_is_erange(L, ptrs):
    scores = np.linspace(0, 1, 5 + 4097, dtype=np.float32)
    cu = np.array([0, 5, 5 + 4097], np.int32)
    args = (scores, cu) if ptrs == "host" else _dev(scores, cu)
    with pytest.raises(L.DIError) as ei:
        L.segment_order(*args)
    assert ei.value.code == -4  # DI_ERANGE


# ------------------------------------------------------------------ end to end
def test_cli_device_route_equals_joined_route_and_reference_loop(L, tmp_path):
    """3 queries x 5 passages (one longer than max_length), local tokenizer, the small
    XLM-R fixture's weights: the CLI's run file with --assemble device == --assemble joined
    == cross_encoder_reranker.py:41-62 restated over the joined route's scores."""
    from improving_learned_index_amd import cross_encoder_rerank  # noqa: F401  (the alias)
    from improving_learned_index_amd.cross_encoder_reranker import CrossEncoderReRanker, main
    from improving_learned_index_amd.models import DeepImpactCrossEncoder

    fx = json.loads((GOLDEN / "encoder_xlmr_small.json").read_text())
    sd = encoder_ref.seeded_state_dict(fx["state_dict_shapes"], fx["seed"], fx["std"])
    torch.save({"model_state_dict": sd}, tmp_path / "best.pt")
    local_tokenizer.save(tmp_path / "tokenizer.json")  # found next to the checkpoint
    rng = np.random.default_rng(1)
    words = local_tokenizer.WORDS
    passages = {str(100 + i): " ".join(rng.choice(words, n)) for i, n in
                enumerate([12, 30, 80, 5, 21, 9, 17, 26])}  # "102": 80 words > 48 tokens
    queries = {"9": "what is a learned sparse index", "4": "water", "11": "neural ranking  model?"}
    cands = {"9": ["100", "101", "102", "103", "104"], "4": ["102", "105", "100", "106", "107"],
             "11": ["107", "106", "102", "101", "105"]}
    (tmp_path / "collection.tsv").write_text(
        "".join(f"{p}\t{t}\n" for p, t in passages.items()), encoding="utf-8")
    (tmp_path / "top.tsv").write_text(
        "".join(f"{q}\t{p}\t{queries[q]}\t{passages[p]}\n" for q in cands for p in cands[q]),
        encoding="utf-8")
    saved = DeepImpactCrossEncoder.tokenizer
    try:
        common = ["--checkpoint_path", str(tmp_path / "best.pt"), "--top_k_path",
                  str(tmp_path / "top.tsv"), "--collection_path", str(tmp_path / "collection.tsv"),
                  "--max_length", "48", "--precision", "fp32"]
        main(common + ["--output_path", str(tmp_path / "run.device.txt")])
        main(common + ["--output_path", str(tmp_path / "run.joined.txt"), "--assemble", "joined",
                       "--batch_size", "4"])
        dev_bytes = (tmp_path / "run.device.txt").read_bytes()
        assert dev_bytes == (tmp_path / "run.joined.txt").read_bytes()

        # the device route really ran (no fall-back to the joined route), also in small steps
        rr = CrossEncoderReRanker(tmp_path / "best.pt", tmp_path / "top.tsv",
                                  tmp_path / "collection.tsv", tmp_path / "run.steps.txt",
                                  batch_size=4, precision="fp32", max_length=48)
        rr.run()
        assert rr.assemble == "device" and rr._checked
        assert (tmp_path / "run.steps.txt").read_bytes() == dev_bytes
        assert rr.rerank("4") == rr.rerank(4)

        # cross_encoder_reranker.py:41-62 + RunFile.writelines, over the joined route's scores
        rj = CrossEncoderReRanker(None, tmp_path / "top.tsv", tmp_path / "collection.tsv",
                                  tmp_path / "unused.txt", model=rr.model, max_length=48,
                                  assemble="joined")
        lines = []
        for qid in rj.top_k.keys():
            top_k_pids = rj.top_k[qid]
            scores = rj._score_joined([(qid, pid) for pid in top_k_pids]).tolist()
            ranked = sorted(zip(top_k_pids, scores), key=lambda x: x[1], reverse=True)
            for rank, (pid, score) in enumerate(ranked, start=1):
                lines.append(f"{qid}\t{pid}\t{rank}\t{score}\n")
        assert "".join(lines).encode("utf-8") == dev_bytes
        assert len(lines) == 15 and lines[0].startswith("9\t")
    finally:
        DeepImpactCrossEncoder.tokenizer = saved
