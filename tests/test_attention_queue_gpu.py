"""attention_x3's unit order (precision "bf16x3"): launch_attn_order sorts a call's documents
by token count, longest first, and the attention launches deal the (document, head) units
along that list -- long documents to the 8-wave kernel, documents of at most 192 tokens to
the 4-wave form.  Which workgroup computes a unit, and in which launch, cannot change the
unit's arithmetic, so every impact must equal, bit for bit, the one of the walk over the
documents as they come (DI_ATTN_X3_QUEUE=0), and match the torch fp32 oracle at the
tolerance of test_bf16x3_ragged_batches_match_torch_oracle.

The knob is read once per process, so each side runs in a fresh child process (this file
run as a script): one child per side encodes every batch below, in turn, on one handle.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
RTOL, ATOL = 1e-3, 1e-6  # test_bf16x3_ragged_batches_match_torch_oracle's
VOCAB = 250002
# the 16-query tile edge, the edge between the two forms (192 | 193), the second-pass
# edge of the 8-wave kernel (384 | 385)
EDGE = [1, 16, 17, 192, 193, 384, 385, 300, 8]


def _lens():
    # many: 700 x 12 heads = 8400 units against at most 512 workgroups
    many = np.random.default_rng(41).integers(8, 41, 700).tolist()
    return {"one": [9], "edge": EDGE, "many": many}


def _batch(name, lens):
    """(pad, mask) of the seeded random batch `name` (<s> first, ids uniform)."""
    rng = np.random.default_rng(sum(lens) + len(name))
    pad = np.ones((len(lens), max(lens)), np.int64)
    mask = np.zeros_like(pad)
    for i, n in enumerate(lens):
        pad[i, :n] = rng.integers(5, VOCAB, n)
        pad[i, 0] = 0
        mask[i, :n] = 1
    return pad, mask


def _pack(pad, mask, rows=None):
    rows = range(len(pad)) if rows is None else rows
    ids = np.concatenate([pad[r, :int(mask[r].sum())] for r in rows]).astype(np.int32)
    cu = np.zeros(len(rows) + 1, np.int32)
    cu[1:] = np.cumsum([int(mask[r].sum()) for r in rows])
    return ids, cu


def _edge_terms():
    """Term selections of the edge batch: document 0 (one token) keeps its token, document
    3 one term, document 8 none; the others a seeded subset."""
    rng = np.random.default_rng(5)
    tt, ct = [], [0]
    for d, n in enumerate(EDGE):
        k = {0: 1, 3: 1, 8: 0}.get(d, int(rng.integers(1, n + 1)))
        tt += np.sort(rng.choice(n, size=k, replace=False)).tolist()
        ct.append(len(tt))
    return np.array(tt, np.int32), np.array(ct, np.int32)


def _base():
    import encoder_ref

    fx = json.loads((ROOT / "tests" / "golden" / "encoder_xlmr_base.json").read_text())
    return fx, encoder_ref.seeded_state_dict(fx["state_dict_shapes"], fx["seed"], fx["std"])


def _child(out_path):
    """Every batch on one handle, in turn; the per-token (or per-term) impacts to out_path."""
    for p in (ROOT, ROOT / "oracle", ROOT / "tests" / "golden"):
        sys.path.insert(0, str(p))
    from improving_learned_index_amd import encoder as E

    fx, sd = _base()
    c = fx["config"]
    cfg = E.EncoderConfig(variant="xlmr", activation="softplus", vocab_size=c["vocab_size"],
                          hidden=c["hidden_size"], layers=c["num_hidden_layers"],
                          heads=c["num_attention_heads"], intermediate=c["intermediate_size"],
                          max_positions=c["max_position_embeddings"],
                          type_vocab=c["type_vocab_size"], pad_id=c["pad_token_id"],
                          layer_norm_eps=c["layer_norm_eps"])
    enc = E.DeviceEncoder(sd, cfg, precision="bf16x3")
    out = {}
    batches = {k: _batch(k, v) for k, v in _lens().items()}
    for name in ("many", "one", "edge"):  # (a larger batch first: its list stays behind)
        ids, cu = _pack(*batches[name])
        out[name] = enc.encode_packed(ids, cu, token_impacts=True)
    pad, mask = batches["edge"]
    ids, cu = _pack(pad, mask)
    # the same handle again: "one" (1 document) after "edge" (9), "edge" after "one"
    ids1, cu1 = _pack(*batches["one"])
    out["one_again"] = enc.encode_packed(ids1, cu1, token_impacts=True)
    out["edge_again"] = enc.encode_packed(ids, cu, token_impacts=True)
    tt, ct = _edge_terms()
    out["edge_terms"] = enc.encode_packed(ids, cu, tt, ct)
    rev = list(range(len(EDGE)))[::-1]
    rids, rcu = _pack(pad, mask, rev)
    out["edge_reversed"] = enc.encode_packed(rids, rcu, token_impacts=True)
    np.savez(out_path, **out)


def _run_child(tmp, name, knob):
    env = dict(os.environ)
    env.pop("DI_ATTN_X3_QUEUE", None)
    if knob is not None:
        env["DI_ATTN_X3_QUEUE"] = knob
    path = tmp / f"{name}.npz"
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), str(path)], env=env,
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        pytest.fail(f"child {name} (DI_ATTN_X3_QUEUE={knob}) ended with {r.returncode}:\n"
                    f"{r.stderr[-2000:]}")
    return dict(np.load(path))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """(with the list -- the default --, one launch per layer, without the list)."""
    from improving_learned_index_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible (GPU test run without a GPU)")
    tmp = tmp_path_factory.mktemp("attn_queue")
    queue = _run_child(tmp, "queue", None)
    one_form = _run_child(tmp, "one_form", "1")
    static = _run_child(tmp, "static", "0")
    return queue, one_form, static


@pytest.fixture(scope="module")
def oracle():
    """The torch fp32 oracle's per-token impacts of every batch, computed once (the 700
    short documents in length-sorted groups of 64: little padding)."""
    import torch

    import encoder_ref

    fx, sd = _base()
    want = {}
    for name, lens in _lens().items():
        pad, mask = _batch(name, lens)
        tok = [None] * len(lens)
        order = np.argsort(lens, kind="stable")
        for s0 in range(0, len(order), 64):
            b = order[s0:s0 + 64]
            w = int(max(lens[d] for d in b))
            with torch.no_grad():
                y = encoder_ref.forward(sd, fx["config"], torch.from_numpy(pad[b, :w]),
                                        torch.from_numpy(mask[b, :w]), "xlmr",
                                        "softplus").numpy()
            for r, d in enumerate(b):
                tok[d] = y[r, :lens[d]]
        want[name] = np.concatenate(tok).astype(np.float32)
    return want


pytestmark = pytest.mark.gpu


def _check(runs, oracle, name):
    queue, one_form, static = runs
    assert queue[name].shape == oracle[name].shape
    np.testing.assert_array_equal(queue[name], static[name])
    np.testing.assert_array_equal(one_form[name], static[name])
    np.testing.assert_allclose(queue[name], oracle[name], rtol=RTOL, atol=ATOL)


def test_fewer_units_than_workgroups(runs, oracle):
    """One document of 9 tokens: 12 units, every other workgroup finds none."""
    _check(runs, oracle, "one")


def test_edge_lengths(runs, oracle):
    _check(runs, oracle, "edge")


def test_more_units_than_workgroups(runs, oracle):
    """700 documents of 8 to 40 tokens: every workgroup takes many units, in both
    directions of the deal."""
    _check(runs, oracle, "many")


def test_list_of_an_earlier_batch_is_not_reused(runs, oracle):
    """On one handle a batch after a larger and after a smaller one: the list and the
    slices are the call's own."""
    queue, one_form, static = runs
    for r in (queue, one_form):
        np.testing.assert_array_equal(r["one_again"], static["one"])
        np.testing.assert_array_equal(r["edge_again"], static["edge"])
    np.testing.assert_array_equal(static["edge_again"], static["edge"])


def test_pruned_last_layer(runs):
    """The edge batch with term selections (one document of one token, one with one kept
    term, one with none): the unpruned rows' impacts, bit for bit."""
    queue, one_form, static = runs
    tt, ct = _edge_terms()
    cu = np.concatenate([[0], np.cumsum(EDGE)])
    rows = np.concatenate([cu[d] + tt[ct[d]:ct[d + 1]] for d in range(len(EDGE))])
    for r in (queue, one_form, static):
        np.testing.assert_array_equal(r["edge_terms"], static["edge"][rows])


def test_document_order_does_not_matter(runs):
    queue, one_form, static = runs
    cu = np.concatenate([[0], np.cumsum(EDGE)])
    want = np.concatenate([static["edge"][cu[d]:cu[d + 1]] for d in range(len(EDGE))[::-1]])
    for r in (queue, one_form, static):
        np.testing.assert_array_equal(r["edge_reversed"], want)


if __name__ == "__main__":
    _child(sys.argv[1])
