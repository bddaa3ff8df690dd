"""GPU parity of the encoder at every kind of model shape di_encoder_create accepts.

The library takes any hidden that is a multiple of 64 up to 1024 (head dim 64), any
intermediate that is a multiple of 64, and bf16x3 at hidden 768 and 1024; the rest of the
suite runs hidden 128 and 768 only.  Each shape here has 2 layers, vocabulary 1024, the
peaked_state_dict weights of tests/encoder_cases.py (tests/test_encoder_cases_cpu.py
proves that they move the softmax's running maximum after the first key block in 3 to 12 %
of the rows, and that the output sees a projection shifted by one head on > 84 % of the
tokens) and documents of 385, 200, 130, 97, 65, 33, 32, 2 and 1 tokens -- 945 rows, an M
tail in both the 128-row and the 256-row GEMM tiles:

  hidden heads interm  reaches
     64     1     64   one head; N and K below one tile
    192     3    320   N % 128 == 64 in all four GEMMs; ln_kernel<4> with H < 256
    256     4    512   bf16 folded, n_part 1; generic embed into the folded path
    384     6   1536   bf16: FFN1 on the 256-tile kernel, the rest on the 128-tile one; PL 12
    512     8   1024   bf16 folded, n_part 2
    832    13    448   PL 16 with H < 1024; odd head count; ragged intermediate
   1024    16   4096   the large shape: *_vec_kernel<., 4>, n_part 4
   1024    16   1280   bf16x3 with an odd number of 256-column FFN tiles

Bounds, each the project's own: fp32 and bf16x3 within 1e-3 relative (atol 1e-6) of the
float64 oracle (the north-star bound of test_encoder_bf16x3_gpu.py); bf16 within |d| <=
0.05 + 0.05 |x| per token with a median relative error < 1e-2 (test_encoder_gpu.py; a
torch emulation on the CPU that rounds every GEMM and attention operand to bf16 gives
median 4.0e-3 / max 2.5e-2 at hidden 1024 with these weights, inside the bound); pruned
term output and a repeated encode: bit for bit.  The bf16 bound is one figure for every
shape, so the bf16 median is also held to twice that of the bf16 storage emulation of the
same shape (encoder_cases assert_bf16_format_bound; 3.7e-4 at hidden 64 to 4.8e-3 at 1024).

Device error against the float64 oracle measured on an MI355X (median / max relative):
  hidden interm  fp32               bf16               bf16x3 folded      bf16x3 unfolded
     64     64   2.8e-08 / 1.2e-07  3.6e-04 / 2.4e-03
    192    320   5.1e-08 / 3.7e-07  7.4e-04 / 4.2e-03
    256    512   7.9e-08 / 7.1e-07  9.4e-04 / 5.0e-03
    384   1536   1.8e-07 / 8.2e-07  1.8e-03 / 8.2e-03
    512   1024   3.0e-07 / 1.9e-06  2.1e-03 / 1.1e-02
    832    448   5.8e-07 / 3.9e-06  3.4e-03 / 2.0e-02
   1024   4096   8.4e-07 / 6.5e-06  4.0e-03 / 2.4e-02  7.0e-06 / 4.4e-05  6.4e-06 / 4.3e-05
   1024   1280   9.3e-07 / 3.9e-06  4.7e-03 / 3.0e-02  8.0e-06 / 5.2e-05  8.3e-06 / 4.4e-05

Two findings of this module, both fixed with it.  Hidden 64 in bf16 measured 7.3e-3 /
7.6e-2 -- inside the bf16 bound, twenty times the format's error: with one head the
attention's pair -> document multiply-high used the magic number 2^32 mod 2^32 = 0, so
every pair computed document 0 (test_shape_matches_float64_oracle[h64-f64-bf16] through
the format bound).  And the pruned last layer packs its gathered rows, hidden wide, into
the FFN buffer, which was sized by the intermediate size alone: with intermediate < hidden
the rows ran past it (the 512 / 256 case of test_shape_pruned_last_layer_is_bitexact; found
by reading, the buffer is sized for both now).
"""
import numpy as np
import pytest

import encoder_cases as C

pytestmark = pytest.mark.gpu

LENS = tuple(C.SHAPE_LENS)
SHAPE_IDS = [f"h{h}-f{f}" for h, f in C.SHAPES]
LARGE = [(1024, 4096), (1024, 1280)]


@pytest.fixture(scope="module")
def E():
    from improving_learned_index_amd import _lib, encoder

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible (GPU test run without a GPU)")
    return encoder


def _case(hidden, intermediate):
    """(state dict, config, packed ids, cu_seqlens, float64 oracle impacts) -- the oracle
    is computed once per shape and shared (C.want), the weights are regenerated."""
    _, cfg, sd, pad, mask = C.case(hidden, intermediate, list(LENS))
    ids, cu = C.pack(pad, mask)
    return sd, cfg, ids, cu, C.want(hidden, intermediate, LENS)


def _report(name, got, want):
    r = C.rel_err(got, want)
    print(f"{name}: relative error median {np.median(r):.2e} max {r.max():.2e}")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("hidden,intermediate", C.SHAPES, ids=SHAPE_IDS)
def test_shape_matches_float64_oracle(E, hidden, intermediate, precision):
    sd, cfg, ids, cu, want = _case(hidden, intermediate)
    enc = E.DeviceEncoder(sd, C.device_config(E, cfg), precision=precision)
    assert enc.precision == precision
    got = enc.encode_packed(ids, cu, token_impacts=True)
    _report(f"hidden {hidden} intermediate {intermediate} {precision}", got, want)
    if precision == "fp32":
        C.assert_fp32_bound(got, want)
    else:
        C.assert_bf16_bound(got, want)
        C.assert_bf16_format_bound(got, want, C.bf16_format_error(hidden, intermediate, LENS))


@pytest.mark.parametrize("fold", [True, False], ids=["folded", "unfolded"])
@pytest.mark.parametrize("hidden,intermediate", LARGE, ids=["h1024-f4096", "h1024-f1280"])
def test_large_shape_bf16x3_matches_float64_oracle(E, monkeypatch, hidden, intermediate, fold):
    sd, cfg, ids, cu, want = _case(hidden, intermediate)
    if not fold:
        monkeypatch.setenv("DI_NO_LN_FOLD", "1")
    enc = E.DeviceEncoder(sd, C.device_config(E, cfg), precision="bf16x3")
    assert enc.precision == "bf16x3"
    got = enc.encode_packed(ids, cu, token_impacts=True)
    _report(f"hidden {hidden} intermediate {intermediate} bf16x3 "
            + ("folded" if fold else "unfolded"), got, want)
    C.assert_fp32_bound(got, want)


@pytest.mark.parametrize("hidden,intermediate", [s for s in C.SHAPES if s not in LARGE],
                         ids=[i for i, s in zip(SHAPE_IDS, C.SHAPES) if s not in LARGE])
def test_bf16x3_request_outside_its_shapes_runs_fp32(E, hidden, intermediate):
    """The wrapper takes the f32 MFMA mode for shapes the split-bf16 kernels do not take;
    the mode that ran is stated (its output is test_shape_matches_float64_oracle[fp32])."""
    shp, cfg = C.shapes(hidden, intermediate)
    enc = E.DeviceEncoder(C.peaked_state_dict(shp, C.SEED), C.device_config(E, cfg),
                          precision="bf16x3")
    assert enc.precision == "fp32"


@pytest.mark.parametrize("hidden,intermediate,precision", [
    (256, 512, "bf16"), (512, 1024, "bf16"), (1024, 4096, "bf16"), (1024, 4096, "bf16x3"),
    (1024, 1280, "bf16x3"), C.NARROW_FFN + ("bf16",)])
def test_shape_pruned_last_layer_is_bitexact(E, hidden, intermediate, precision):
    """Term output (last layer on the terms' rows only; bf16 runs it when folded) equals
    the per-token output gathered at the term rows, bit for bit: a document without
    terms, all tokens of the 385-token document, repeated positions, unsorted order."""
    sd, cfg, ids, cu, _ = _case(hidden, intermediate)
    enc = E.DeviceEncoder(sd, C.device_config(E, cfg), precision=precision)
    assert enc.precision == precision
    tok = enc.encode_packed(ids, cu, token_impacts=True)
    tt, ct = C.random_terms(np.random.default_rng(hidden), LENS)
    assert ct[-1] <= cu[-1]  # (more term rows than tokens would turn the pruning off)
    # (intermediate < hidden: the packed term rows take more than the FFN buffer's
    # intermediate-wide rows of the batch -- it is sized for them)
    assert (hidden, intermediate) != C.NARROW_FFN or ct[-1] * hidden > 1024 * intermediate
    want = np.array([tok[cu[d] + tt[j]] for d in range(len(LENS)) for j in range(ct[d], ct[d + 1])],
                    np.float32)
    np.testing.assert_array_equal(enc.encode_packed(ids, cu, tt, ct), want)


def test_workspace_reuse_fp32_hidden_192(E):
    """One encoder: the full batch, its last three documents (32, 2 and 1 tokens), the
    full batch again -- the workspace keeps its size while the V^T leading dimension and
    column layout change with the batch.  Each result within the fp32 bound of the oracle,
    the first and the third bit-identical."""
    sd, cfg, ids, cu, want = _case(192, 320)
    enc = E.DeviceEncoder(sd, C.device_config(E, cfg), precision="fp32")
    first = enc.encode_packed(ids, cu, token_impacts=True).copy()
    t0 = cu[-4]
    tail = enc.encode_packed(ids[t0:], cu[-4:] - t0, token_impacts=True).copy()
    third = enc.encode_packed(ids, cu, token_impacts=True).copy()
    C.assert_fp32_bound(first, want)
    C.assert_fp32_bound(tail, want[t0:])
    C.assert_fp32_bound(third, want)
    np.testing.assert_array_equal(first, third)


@pytest.mark.parametrize("hidden,heads,intermediate", [(192, 2, 320), (192, 4, 320),
                                                       (1088, 17, 1024), (192, 3, 96)],
                         ids=["head-dim-96", "head-dim-48", "hidden-1088", "intermediate-96"])
def test_rejected_configurations(E, hidden, heads, intermediate):
    from improving_learned_index_amd import _lib

    shp, cfg = C.shapes(hidden, intermediate, layers=1)
    cfg["num_attention_heads"] = heads
    sd = C.peaked_state_dict(shp, C.SEED)
    for precision in ("fp32", "bf16"):
        with pytest.raises(_lib.DIError):
            E.DeviceEncoder(sd, C.device_config(E, cfg), precision=precision)
