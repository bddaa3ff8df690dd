"""What the inputs of test_encoder_peaked_gpu.py and test_encoder_shapes_gpu.py can see,
proved from the CPU oracle alone (oracle/encoder_ref.py; no GPU).

With seeded_state_dict(std 0.02) weights the attention logits stay under ~2, so no softmax
row of any existing encoder test moves the device's lazy reference maximum after the first
key chunk (enc_attn_x3.hip soft_a: rescale when a score passes the reference by 8 in base 2),
and shifting K by one head moves the impacts by about the suite's 1e-3 bound.  The
peaked_state_dict weights of tests/encoder_cases.py (logit standard deviation 6, value /
output projections doubled) are held to three conditions here, for every (shape, lens) the
two GPU modules use; a seed or lens that misses one is changed, the thresholds are not:

  1. rescale rows: in every layer, the fraction of (document, head, query) rows where a
     later key block exceeds all earlier blocks by more than 8 ln 2 is >= 0.03 at 32-key
     blocks and >= 0.02 at 64-key blocks (a lower bound on the device's rescale events).
     Measured, layer 0 / layer 1, seed 7:
       hidden  interm   block 32       block 64
          64      64   0.069 0.125    0.041 0.074
         192     320   0.116 0.069    0.057 0.039
         256     512   0.067 0.075    0.044 0.059
         384    1536   0.075 0.090    0.056 0.044
         512    1024   0.103 0.075    0.056 0.043
         832     448   0.083 0.056    0.045 0.032
        1024    4096   0.103 0.062    0.062 0.031
        1024    1280   0.087 0.055    0.048 0.028
         768    3072   0.112 0.069    0.068 0.043   (the peaked module's lens)
     The largest |logit| is 26 to 40.  (Hidden 512 / intermediate 256, the narrow-FFN case
     of the pruned-layer test, is held to the same conditions.)
  2. head sensitivity (hidden >= 128): with the query, key or value projection rolled by
     one head, the oracle's impact differs by more than 1e-2 relative (10x the fp32 /
     bf16x3 bound) on >= 60 % of the tokens.  Measured 0.85 (hidden 192) to 0.99 (hidden
     1024) for each of the three.
  3. contrast: the plain seeded weights give 0 rescale rows at both block sizes.

layer_logits is a restatement of the oracle's forward; its impacts are held to
encoder_ref.forward's (float32 against float64: measured <= 3.4e-6 relative, bound 2e-5).
"""
import numpy as np
import pytest
import torch

import encoder_cases as C
import encoder_ref

CASES = [(h, f, tuple(C.SHAPE_LENS)) for h, f in C.SHAPES + [C.NARROW_FFN]] + [
    (768, 3072, tuple(C.PEAKED_LENS))]
IDS = [f"h{h}-f{f}" for h, f, _ in CASES]


@pytest.fixture(autouse=True)
def _torch_on_one_thread():
    """(the tests' own torch operations too: see encoder_cases._one_torch_thread)"""
    with C._one_torch_thread():
        yield


def _case(hidden, intermediate, lens):
    """The case (regenerated: only the float64 oracle's impacts are kept between tests)."""
    return C.case(hidden, intermediate, list(lens)) + (C.want(hidden, intermediate, lens),)


@pytest.mark.parametrize("hidden,intermediate,lens", CASES, ids=IDS)
def test_peaked_weights_move_the_running_maximum(hidden, intermediate, lens):
    shp, cfg, sd, pad, mask, want = _case(hidden, intermediate, lens)
    logits, imp = C.layer_logits(sd, cfg, pad, mask)
    assert len(logits) == cfg["num_hidden_layers"] == 2
    assert logits[0].shape == (len(lens), hidden // 64, max(lens), max(lens))
    # the restatement is the oracle
    np.testing.assert_allclose(imp, want, rtol=2e-5, atol=0)
    r32 = [C.rescale_rows(l, lens, 32) for l in logits]
    r64 = [C.rescale_rows(l, lens, 64) for l in logits]
    print(f"rescale rows block 32 {np.round(r32, 3)} block 64 {np.round(r64, 3)}")
    assert min(r32) >= 0.03, r32
    assert min(r64) >= 0.02, r64


@pytest.mark.parametrize("hidden,intermediate,lens", CASES, ids=IDS)
def test_plain_seeded_weights_never_rescale(hidden, intermediate, lens):
    shp, cfg, _, pad, mask, _ = _case(hidden, intermediate, lens)
    sd = encoder_ref.seeded_state_dict(shp, C.SEED, 0.02)
    logits, _ = C.layer_logits(sd, cfg, pad, mask)
    assert [C.rescale_rows(l, lens, b) for l in logits for b in (32, 64)] == [0.0] * 4


@pytest.mark.parametrize("which", ["query", "key", "value"])
@pytest.mark.parametrize("hidden,intermediate,lens", [c for c in CASES if c[0] >= 128],
                         ids=[i for i, c in zip(IDS, CASES) if c[0] >= 128])
def test_output_sees_a_one_head_shift(hidden, intermediate, lens, which):
    _, cfg, sd, pad, mask, want = _case(hidden, intermediate, lens)
    got = C.oracle(C.roll_heads(sd, which), cfg, pad, mask, dtype=torch.float32)
    frac = C.sensitive_fraction(want, got, 1e-2)
    print(f"{which} rolled by one head: {frac:.3f} of the tokens move by > 1e-2")
    assert frac >= 0.60, frac


@pytest.mark.parametrize("hidden,intermediate,lens", CASES, ids=IDS)
def test_bf16_storage_emulation_is_inside_the_bf16_bound(hidden, intermediate, lens):
    """The reference side of the bf16 checks: the forward with every stored tensor rounded
    to bf16 meets the project's bf16 bound, and its median error (the figure the GPU tests
    hold the device's to, within a factor 2) grows with the hidden size as a rounding
    error does -- 3.7e-4 at hidden 64, 3.1e-3 at 768, 4.6e-3 at 1024."""
    _, cfg, sd, pad, mask, want = _case(hidden, intermediate, lens)
    got = C.oracle_bf16_storage(sd, cfg, pad, mask)
    r = C.rel_err(got, want)
    print(f"bf16 storage emulation: relative error median {np.median(r):.2e} max {r.max():.2e}")
    C.assert_bf16_bound(got, want)
    assert 1e-4 < np.median(r) < 5e-3


def test_rescale_rows_counts_by_hand():
    """Two documents, one head: only the 5-token document is longer than the block of 4;
    its query 0 has key 4 (block 1) 6 above block 0's maximum (> 8 ln 2 = 5.55), query 1
    only 5 above, the others nothing -> 1 of 5 rows."""
    s = torch.zeros(2, 1, 5, 5)
    s[0, 0, 0, 4] = 6.0
    s[0, 0, 1, 4] = 5.0
    s[1] = 100.0 * torch.arange(5.0)  # a 4-token document: not longer than the block
    assert C.rescale_rows(s, [5, 4], 4) == pytest.approx(1 / 5)
    assert C.rescale_rows(s, [5, 4], 8) == 0.0
    # block 2: document 1 counts too, and each of its 4 rows climbs by 200 into block 1
    assert C.rescale_rows(s, [5, 4], 2) == pytest.approx((1 + 4) / 9)


def test_shapes_and_roll():
    shp, cfg = C.shapes(192, 320)
    d = {k: s for k, s, _ in shp}
    assert cfg["num_attention_heads"] == 3 and cfg["num_hidden_layers"] == 2
    assert d["bert.embeddings.word_embeddings.weight"] == [1024, 192]
    assert d["bert.embeddings.position_embeddings.weight"] == [514, 192]
    assert d["bert.encoder.layer.1.intermediate.dense.weight"] == [320, 192]
    assert d["bert.encoder.layer.1.output.dense.weight"] == [192, 320]
    assert not any(".layer.2." in k for k in d)
    sd = C.peaked_state_dict(shp, 7)
    base = encoder_ref.seeded_state_dict(shp, 7, 0.02)
    k = "bert.encoder.layer.0.attention.self.key."
    assert float(sd[k + "weight"].std()) == pytest.approx((6.0 / 192) ** 0.5, rel=0.02)
    assert torch.equal(sd[k + "bias"], base[k + "bias"])
    assert torch.equal(sd["bert.encoder.layer.1.attention.self.value.weight"],
                       2.0 * base["bert.encoder.layer.1.attention.self.value.weight"])
    r = C.roll_heads(sd, "key")
    assert torch.equal(r[k + "weight"][64:128], sd[k + "weight"][:64])
    assert torch.equal(r[k + "bias"][:64], sd[k + "bias"][128:])
    q = "bert.encoder.layer.0.attention.self.query.weight"
    assert r[q] is sd[q]
