"""di_encode_pairwise on the GPU: DeepPairwiseImpact's pair attentions and pair scores
(reference src/deep_impact/models/pairwise_impact.py:20-95) against the float64 oracle of
tests/pairwise_cases.py, in every supported precision; the singles, batch invariance, the
edges of the call and `index --pairwise` end to end.

Criteria.  attn: the project's north-star bound, rtol 1e-3 / atol 1e-6.  Pair scores:
|got - want| <= 1e-3 want + atol with atol = 4 x the largest pair-score error of the
precision's CPU storage emulation (pairwise_cases.pair_atol: u_a + v_b cancels and the
ReLU puts scores next to zero, so the relative part cannot stand alone); atol is about
1.7e-5 for fp32 and 2.0e-4 for bf16x3 on the 768 inputs, below half a printed step."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import encoder_cases as C
import encoder_ref
import pairwise_cases as P
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

PRECS = ["fp32", "bf16x3", "bf16x3-nofold"]


def _make_encoder(sd, cfg, prec):
    from improving_learned_index_amd import encoder as E

    nofold = prec.endswith("-nofold")
    old = os.environ.pop("DI_NO_LN_FOLD", None)
    if nofold:
        os.environ["DI_NO_LN_FOLD"] = "1"
    try:
        return E.DeviceEncoder(sd, P.device_config(E, cfg), precision=prec.split("-")[0])
    finally:
        os.environ.pop("DI_NO_LN_FOLD", None)
        if old is not None:
            os.environ["DI_NO_LN_FOLD"] = old


@functools.lru_cache(maxsize=None)
def encoder(prec, shape=(768, 3072, P.LENS)):
    from improving_learned_index_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible (GPU test run without a GPU)")
    cfg, sd, *_ = P.inputs(*shape)
    return _make_encoder(sd, cfg, prec)


@functools.lru_cache(maxsize=None)
def device_result(prec, shape=(768, 3072, P.LENS)):
    """(single, pair, cu_pairs, attn) of the shared inputs, once per precision."""
    _, _, pad, mask, tt, ct = P.inputs(*shape)
    ids, cu = C.pack(pad, mask)
    out = encoder(prec, shape).encode_pairwise(ids, cu, tt, ct, attentions=True)
    for a in out:
        a.setflags(write=False)
    return out


def _check_attn(got, want):
    rel = np.abs(got - want) / np.abs(want)
    print(f"attn relative error: median {np.median(rel):.3g} max {rel.max():.3g}")
    np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-6)


def _check_scores(got, want_pre, want, atol):
    err = np.abs(got - want)
    print(f"pair scores: atol {atol:.3g}; max |err| {err.max():.3g}; "
          f"max (|err| - 1e-3 want) {(err - 1e-3 * want).max():.3g}; "
          f"positive on the device {np.mean(got > 0):.3f}")
    assert (err <= 1e-3 * want + atol).all(), float((err - 1e-3 * want).max())
    sure_zero = want_pre < -atol
    assert sure_zero.any() and (got[sure_zero] == 0).all()


@pytest.mark.parametrize("prec", PRECS)
def test_pair_attentions_against_float64(prec):
    """Measured relative error, median / max (printed by every run): fp32 2.4e-6 / 3.3e-5,
    bf16x3 2.2e-5 / 4.6e-4, bf16x3 unfolded 2.1e-5 / 3.5e-4; the CPU storage emulations
    give max 2.7e-5 (float32) and 2.6e-4 (split 16 bits)."""
    _, pair, cu_pairs, attn = device_result(prec)
    want = P.oracle()["full"][1]
    assert len(attn) == len(want) == 3601 and cu_pairs[-1] == 3601
    _check_attn(attn, want)


@pytest.mark.parametrize("prec", PRECS)
def test_pair_scores_against_float64(prec):
    """Measured: atol 1.6e-5 (fp32; 1.7e-5 with another CPU's float32 forward) and 2.0e-4
    (bf16x3); max |err| 4.8e-6 / 6.0e-5 / 6.0e-5, max (|err| - 1e-3 want) 1.8e-6 / 2.9e-5 /
    3.6e-5 for fp32 / bf16x3 / bf16x3 unfolded."""
    _, pair, _, _ = device_result(prec)
    _, _, pre, want = P.oracle()["full"]
    _check_scores(pair, pre, want, P.pair_atol(prec.split("-")[0]))


def test_fp32_three_heads_small_shape():
    """hidden 192 / intermediate 320: a mean over 3 heads on a shape outside the 256-tile
    path; lengths 65, 33 and 2."""
    _, pair, _, attn = device_result("fp32", P.SMALL)
    _, wattn, pre, want = P.oracle(*P.SMALL)["full"]
    _check_attn(attn, wattn)
    _check_scores(pair, pre, want, P.pair_atol("fp32", *P.SMALL))


@pytest.mark.parametrize("prec", ["bf16x3", "fp32"])
def test_singles_are_di_encodes(prec):
    from improving_learned_index_amd.models import round3

    _, _, pad, mask, tt, ct = P.inputs()
    ids, cu = C.pack(pad, mask)
    enc = encoder(prec)
    before = enc.encode_packed(ids, cu, tt, ct).copy()
    single, pair, _, _ = device_result(prec)
    s2, p2, _ = enc.encode_pairwise(ids, cu, tt, ct)
    after = enc.encode_packed(ids, cu, tt, ct)
    assert before.tobytes() == single.tobytes() == s2.tobytes() == after.tobytes()
    assert p2.tobytes() == pair.tobytes()
    assert (single > 0).any()
    sr, pr, _ = enc.encode_pairwise(ids, cu, tt, ct, round3=True)
    assert sr.tobytes() == round3(single).tobytes()
    assert pr.tobytes() == round3(pair).tobytes()
    assert (pr != pair).any()


@pytest.mark.parametrize("prec", ["bf16x3", "fp32"])
def test_batch_invariance(prec):
    _, _, pad, mask, tt, ct = P.inputs()
    single, pair, cu_pairs, attn = device_result(prec)
    enc = encoder(prec)
    for d in (0, 2, 6):  # 512, 65 and 2 tokens
        ids, cu = C.pack(pad[d:d + 1], mask[d:d + 1])
        t = tt[ct[d]:ct[d + 1]]
        s1, p1, cp1, a1 = enc.encode_pairwise(ids, cu, t, np.array([0, len(t)], np.int32),
                                              attentions=True)
        assert len(p1) == cp1[-1] == len(t) * (len(t) - 1) // 2
        assert s1.tobytes() == single[ct[d]:ct[d + 1]].tobytes()
        assert p1.tobytes() == pair[cu_pairs[d]:cu_pairs[d + 1]].tobytes()
        assert a1.tobytes() == attn[cu_pairs[d]:cu_pairs[d + 1]].tobytes()


def test_edges_and_refused_calls():
    from improving_learned_index_amd import _lib
    from improving_learned_index_amd import encoder as E

    cfg, sd, pad, mask, tt, ct = P.inputs()
    ids, cu = C.pack(pad, mask)
    enc = encoder("bf16x3")
    good = device_result("bf16x3")

    def still_right():
        s, p, _ = enc.encode_pairwise(ids, cu, tt, ct)
        assert s.tobytes() == good[0].tobytes() and p.tobytes() == good[1].tobytes()

    # every document with at most one term: no pairs, the singles still those of di_encode
    t1 = np.array([3, 0, 64, 0], np.int32)
    c1 = np.array([0, 1, 2, 3, 3, 3, 3, 3, 4], np.int32)
    s, p, cp = enc.encode_pairwise(ids, cu, t1, c1)
    assert len(p) == 0 and (cp == 0).all()
    assert s.tobytes() == enc.encode_packed(ids, cu, t1, c1).tobytes()
    # no documents
    s, p, cp = enc.encode_pairwise(np.zeros(0, np.int32), np.zeros(1, np.int32),
                                   np.zeros(0, np.int32), np.zeros(1, np.int32))
    assert len(s) == 0 and len(p) == 0 and cp.tolist() == [0]
    still_right()
    # term_tok descending inside one document
    bad = tt.copy()
    bad[ct[1]], bad[ct[1] + 1] = tt[ct[1] + 1], tt[ct[1]]
    with pytest.raises(_lib.DIError) as e:
        enc.encode_pairwise(ids, cu, bad, ct)
    assert e.value.code == -1 and "ascending" in str(e.value)
    still_right()
    # a wrong cu_pairs
    T = np.diff(ct.astype(np.int64))
    cp = np.concatenate([[0], np.cumsum(T * (T - 1) // 2)])
    cp[2:] += 1
    with pytest.raises(_lib.DIError) as e:
        enc.encode_pairwise(ids, cu, tt, ct, cu_pairs=cp)
    assert e.value.code == -1 and "cu_pairs" in str(e.value)
    still_right()
    # an encoder without the pair head; a bf16 encoder
    plain = {k: v for k, v in sd.items() if not k.startswith("pairwise_")}
    for w, prec, word in ((plain, "bf16x3", "pairwise_impact_score_encoder"),
                          (sd, "bf16", "bf16")):
        other = E.DeviceEncoder(w, P.device_config(E, cfg), precision=prec)
        want = other.encode_packed(ids, cu, tt, ct).copy()
        with pytest.raises(_lib.DIError) as e:
            other.encode_pairwise(ids, cu, tt, ct)
        assert e.value.code == -1 and word in str(e.value)
        assert other.encode_packed(ids, cu, tt, ct).tobytes() == want.tobytes()
        other.close()
    # one tensor of the pair head without the other, or a wrong shape
    half = {k: v for k, v in sd.items() if k != "pairwise_impact_score_encoder.0.bias"}
    short = dict(sd)
    short["pairwise_impact_score_encoder.0.weight"] = torch.zeros(1, 2 * 768)
    for w in (half, short):
        with pytest.raises(_lib.DIError) as e:
            E.DeviceEncoder(w, P.device_config(E, cfg), precision="bf16x3")
        assert e.value.code == -1


PASSAGES = [
    "the learned sparse retrieval model computes an impact score",
    "search engines index passages and queries hit the inverted index",
    "a very long passage about water and earth and the sea",
    "hello world it is ok",
    "the model computes a score about water",
    "queries about the sea and the earth",
    "sparse retrieval of passages",
    "an inverted index of impact scores",
    "the world of search engines",
    "learned model and learned index",
    "water earth sea world",
    "passages hit the index",
    "numbers and symbols and text",
    "a long text about retrieval",
    "the impact of the model",
    "engines and queries",
    "hello sea",
    "single",
    "ok ok ok world",
    "the very sparse earth",
]


def test_index_pairwise_cli_end_to_end(tmp_path):
    """index --pairwise writes the reference's lines for the encoder's own arrays, and the
    file goes through quantize, index create and rank --pairwise."""
    from improving_learned_index_amd import index as index_cli
    from improving_learned_index_amd.inverted_index import InvertedIndexCreator
    from improving_learned_index_amd.models import DeepPairwiseImpact
    from improving_learned_index_amd.quantize import quantize_file
    from improving_learned_index_amd.ranker import Ranker

    fx = json.loads((GOLDEN / "encoder_xlmr_small.json").read_text())
    sd = encoder_ref.seeded_state_dict(fx["state_dict_shapes"], fx["seed"], fx["std"])
    H = fx["config"]["hidden_size"]
    w = np.random.default_rng(P.PAIR_SEED).standard_normal(2 * H + 1) * 0.05
    w[0] = 4.0
    sd["pairwise_impact_score_encoder.0.weight"] = torch.from_numpy(
        w.astype(np.float32).reshape(1, -1))
    sd["pairwise_impact_score_encoder.0.bias"] = torch.zeros(1)
    ckpt = tmp_path / "DeepPairwiseImpact_latest.pt"
    torch.save({"model_state_dict": sd}, ckpt)
    coll = tmp_path / "collection.tsv"
    coll.write_text("".join(f"{i}\t{t}\n" for i, t in enumerate(PASSAGES)))
    out = tmp_path / "collection.index"
    n = index_cli.run(coll, "msmarco", out, str(ckpt), num_processes=1, process_batch_size=7,
                      tokenizer_path=GOLDEN / "tokenizer.json", max_length=fx["max_length"],
                      precision="fp32", pairwise=True)
    assert n == len(PASSAGES)
    # the same encoder's arrays through the restated compute_term_impacts and line format
    model = DeepPairwiseImpact.load(ckpt, tokenizer_path=GOLDEN / "tokenizer.json",
                                    precision="fp32", max_length=fx["max_length"])
    assert model.encoder.cfg.activation == "relu"
    proc = model.process_documents(PASSAGES, fx["max_length"])
    ids, cu, terms, tt, ct = model.pack_processed(proc)
    single, pair, cu_pairs = model.encoder.encode_pairwise(ids, cu, tt, ct)
    maps = [m for _, m in proc]
    tok = [{i: single[ct[d] + k] for k, i in enumerate(m.values())} for d, m in enumerate(maps)]
    docs = P.restated_term_impacts(maps, tok, [pair[cu_pairs[d]:cu_pairs[d + 1]]
                                                for d in range(len(maps))])
    assert out.read_text() == P.restated_lines(docs)
    # (the tokenizer-pool route of the Indexer formats packed batches)
    assert model.encode_packed_impacts(model.pack_processed_blob(proc))() == out.read_text()
    n_pair_entries = sum("|" in t for d in docs for t, _ in d)
    assert 0 < n_pair_entries < len(pair)  # some pairs are kept, some round to 0.000
    # the reference protocol gives the same numbers
    pad = np.ones((len(proc), max(len(e.ids) for e, _ in proc)), np.int64)
    mask = np.zeros_like(pad)
    for d, (e, _) in enumerate(proc):
        pad[d, :len(e.ids)], mask[d, :len(e.ids)] = e.ids, 1
    from itertools import combinations
    outputs = model(torch.from_numpy(pad), torch.from_numpy(mask), None,
                    [list(combinations(sorted(m.values()), 2)) for m in maps])
    assert np.concatenate([x.numpy().reshape(-1) for x in outputs[1]]).tobytes() == pair.tobytes()
    assert model.compute_term_impacts(maps, outputs) == docs
    # quantize -> index create -> rank --pairwise on that file
    quantize_file(out, tmp_path / "collection.quantized")
    InvertedIndexCreator(tmp_path / "collection.quantized", tmp_path / "index").run()
    # a query made of two terms of one passage whose pair entry survived quantization
    qlines = (tmp_path / "collection.quantized").read_text().split("\n")
    pick = None
    for d, line in enumerate(qlines):
        for part in (line.split(", ") if line else []):
            k, v = part.rsplit(": ", 1)
            if "|" in k and int(v) > 0:
                pick = (d, k, int(v))
                break
        if pick:
            break
    assert pick is not None
    d, key, val = pick
    t1, t2 = key.split("|")
    (tmp_path / "q.tsv").write_text(f"q0\t{t1.lstrip('▁')} {t2.lstrip('▁')}\n")
    posting = dict(p.rsplit(": ", 1) for p in qlines[d].split(", "))
    terms_q = DeepPairwiseImpact.process_query(f"{t1.lstrip('▁')} {t2.lstrip('▁')}")
    assert {t1, t2} == terms_q
    want = sum(int(posting.get(k, 0)) for k in (t1, t2, f"{t1}|{t2}", f"{t2}|{t1}"))
    for pairwise in (True, False):
        Ranker(tmp_path / "index", tmp_path / "q.tsv", tmp_path / "run.tsv", pairwise=pairwise,
               tokenizer_path=GOLDEN / "tokenizer.json").run()
        rows = [l.split("\t") for l in (tmp_path / "run.tsv").read_text().splitlines()]
        score = {int(r[1]): float(r[3]) for r in rows}
        if pairwise:
            assert score[d] == want  # the singles plus the t1|t2 posting
        else:
            assert score[d] == want - val
