"""GPU parity of the encoder at the base shape under peaked attention.

Hidden 768 / 12 heads / intermediate 3072, 2 layers, vocabulary 1024, the
peaked_state_dict weights of tests/encoder_cases.py: logits of standard deviation ~6
(largest |logit| 32 to 35), so that the online softmax of the attention kernels leaves its
first-chunk state -- the lazy reference maximum moves and `lsum` / `o` are rescaled after
the first key chunk, `p` reaches the 2^8 regime, and the row's largest score falls into a
masked partial chunk.  tests/test_encoder_cases_cpu.py proves from the CPU oracle that
these inputs do that (rows that must rescale: 0.112 / 0.069 of all rows at 32-key blocks,
0.068 / 0.043 at 64-key blocks, layer 0 / 1; none with the plain seeded weights) and that
the output sees a projection shifted by one head (> 1e-2 relative on 0.97 of the tokens).

Documents of 512, 385, 384, 257, 256, 65, 64, 33, 32, 17 and 1 tokens: the 384-query pass
edge, the 32- and 64-key chunk edges, a document above 320 tokens (single-buffer bf16
attention) and a single token.

Bounds, each the project's own:
  * fp32 and bf16x3 (LayerNorms folded, and DI_NO_LN_FOLD=1): 1e-3 relative (atol 1e-6)
    of the float64 oracle -- the north-star bound of test_encoder_bf16x3_gpu.py.
  * bf16 (folded, and DI_NO_LN_FOLD=1): |d| <= 0.05 + 0.05 |x| per token and median
    relative error < 1e-2 -- the bf16 bound of test_encoder_gpu.py.  A torch emulation on
    the CPU that rounds every GEMM and attention operand to bf16 gives median 3.0e-3 and
    max 1.6e-2 at these weights, so the reference side is inside the bound.  On top of
    it the median is held to twice the bf16 storage emulation's (encoder_cases
    assert_bf16_format_bound: 3.05e-3 on the CPU here).
  * pruned last layer and batch invariance: bit for bit.

Device error against the float64 oracle measured on an MI355X (median / max relative):
    fp32             5.1e-07 / 2.9e-06
    bf16x3 folded    5.0e-06 / 3.1e-05      unfolded  5.0e-06 / 3.6e-05
    bf16   folded    3.2e-03 / 1.8e-02      unfolded  3.1e-03 / 1.9e-02

test_peaked_pruned_last_layer_is_bitexact found the attention kernels' lazy rescale taken
per 16-query tile: a row whose tile-mate passed its limit moved its own reference maximum
too, so its bits depended on which queries shared the tile, and the pruned last layer
(which regroups the queries) differed from the full one by up to 7e-6 (bf16x3) and 2.9e-3
(bf16) relative.  The decision is per query now.
"""
import numpy as np
import pytest

import encoder_cases as C

pytestmark = pytest.mark.gpu

HIDDEN, INTER = 768, 3072
LENS = tuple(C.PEAKED_LENS)


@pytest.fixture(scope="module")
def E():
    from improving_learned_index_amd import _lib, encoder

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible (GPU test run without a GPU)")
    return encoder


@pytest.fixture(scope="module")
def peaked():
    """(state dict, config, packed ids, cu_seqlens, float64 oracle impacts); read only."""
    _, cfg, sd, pad, mask = C.case(HIDDEN, INTER, list(LENS))
    ids, cu = C.pack(pad, mask)
    return sd, cfg, ids, cu, C.want(HIDDEN, INTER, LENS)


def _report(name, got, want):
    r = C.rel_err(got, want)
    print(f"{name}: relative error median {np.median(r):.2e} max {r.max():.2e}")


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_peaked_matches_float64_oracle(E, peaked, precision):
    sd, cfg, ids, cu, want = peaked
    enc = E.DeviceEncoder(sd, C.device_config(E, cfg), precision=precision)
    assert enc.precision == precision
    got = enc.encode_packed(ids, cu, token_impacts=True)
    _report(precision, got, want)
    C.assert_fp32_bound(got, want)


def test_peaked_bf16x3_unfolded_matches_float64_oracle(E, peaked, monkeypatch):
    """DI_NO_LN_FOLD=1: the split forward with f32 LayerNorm passes (forward_split)."""
    sd, cfg, ids, cu, want = peaked
    monkeypatch.setenv("DI_NO_LN_FOLD", "1")
    enc = E.DeviceEncoder(sd, C.device_config(E, cfg), precision="bf16x3")
    got = enc.encode_packed(ids, cu, token_impacts=True)
    _report("bf16x3 unfolded", got, want)
    C.assert_fp32_bound(got, want)


@pytest.mark.parametrize("fold", [True, False], ids=["folded", "unfolded"])
def test_peaked_bf16_within_bf16_bound(E, peaked, monkeypatch, fold):
    sd, cfg, ids, cu, want = peaked
    if not fold:
        monkeypatch.setenv("DI_NO_LN_FOLD", "1")
    enc = E.DeviceEncoder(sd, C.device_config(E, cfg), precision="bf16")
    got = enc.encode_packed(ids, cu, token_impacts=True)
    _report("bf16 " + ("folded" if fold else "unfolded"), got, want)
    C.assert_bf16_bound(got, want)
    C.assert_bf16_format_bound(got, want, C.bf16_format_error(HIDDEN, INTER, LENS))


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_peaked_pruned_last_layer_is_bitexact(E, peaked, precision):
    """Term output runs the last layer for the terms' rows only (bf16x3: the 4-wave,
    32-key-chunk attention, covered by the rescale rows at block 32); it must equal the
    per-token output gathered at those rows, bit for bit: a document without terms, all
    tokens of the 512-token document, repeated positions, unsorted order."""
    sd, cfg, ids, cu, _ = peaked
    enc = E.DeviceEncoder(sd, C.device_config(E, cfg), precision=precision)
    tok = enc.encode_packed(ids, cu, token_impacts=True)
    tt, ct = C.random_terms(np.random.default_rng(12), LENS)
    assert ct[-1] <= cu[-1]  # (more term rows than tokens would turn the pruning off)
    want = np.array([tok[cu[d] + tt[j]] for d in range(len(LENS)) for j in range(ct[d], ct[d + 1])],
                    np.float32)
    np.testing.assert_array_equal(enc.encode_packed(ids, cu, tt, ct), want)


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_peaked_batch_invariance(E, peaked, precision):
    """Every row's arithmetic is independent of the other documents: the documents of
    512, 257, 33 and 1 tokens encoded alone equal their slices of the batch result."""
    sd, cfg, ids, cu, _ = peaked
    enc = E.DeviceEncoder(sd, C.device_config(E, cfg), precision=precision)
    full = enc.encode_packed(ids, cu, token_impacts=True).copy()
    for n in (512, 257, 33, 1):
        d = LENS.index(n)
        alone = enc.encode_packed(ids[cu[d]:cu[d + 1]], np.array([0, n], np.int32),
                                  token_impacts=True)
        np.testing.assert_array_equal(alone, full[cu[d]:cu[d + 1]], err_msg=f"document of {n}")
