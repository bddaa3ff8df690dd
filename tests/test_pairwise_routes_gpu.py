"""The launch routes of di_encode_pairwise that tests/test_pairwise_gpu.py's one batch does
not reach, each on the smallest inputs that reach it (pairwise_cases.ROUTE_CASES; what
those inputs can show is proven in tests/test_pairwise_cases_cpu.py): more than 8 and more
than 256 documents, 300 terms in one document, 1 / 13 / 16 heads, 4 layers, the BERT
variant that the reference's class is, the device-pointer call with its device-side
checks, the largest document the LDS panel admits, and a workspace that grows and is used
small again.

Criteria, the project's own: attn rtol 1e-3 / atol 1e-6; pair scores |err| <= 1e-3 want +
pair_atol(precision, case) with exact zeros where the oracle is surely negative; singles
byte-equal to encode_packed.

Measured on an MI355X (printed by every run) -- attn relative error median / max; pair
scores atol, max |err|, max (|err| - 1e-3 want):
  many_docs     fp32           9.8e-7 / 1.3e-5;  2.3e-5, 4.7e-6, 8.0e-7
  many_docs_x3  bf16x3         9.1e-6 / 1.5e-4;  2.0e-4, 5.0e-5, 2.5e-5
  many_docs_x3  bf16x3 nofold  9.1e-6 / 1.6e-4;  2.0e-4, 6.4e-5, 3.9e-5
  wide          fp32           3.7e-6 / 4.6e-5;  2.4e-5, 1.0e-5, 5.2e-6
  wide          bf16x3         3.2e-5 / 4.7e-4;  3.6e-4, 9.9e-5, 8.3e-5
  wide          bf16x3 nofold  3.2e-5 / 4.5e-4;  3.6e-4, 9.4e-5, 7.1e-5
  heads64       fp32           1.1e-6 / 8.6e-6;  3.2e-5, 5.2e-6, 2.2e-8
  heads832      fp32           2.6e-6 / 4.0e-5;  2.1e-5, 6.9e-6, 1.2e-6
  layers4       fp32           1.1e-6 / 1.6e-5;  2.3e-5, 4.6e-6, 9.4e-7
  bert          fp32           1.5e-6 / 2.0e-5;  1.1e-5, 5.1e-6, 0
  bert          bf16x3         1.5e-5 / 2.6e-4;  1.7e-4, 4.6e-5, 1.9e-5
  long          fp32           1.6e-6 / 9.3e-6;  1.3e-5, 2.9e-6, 0
(the fp32 atol comes from the float32 forward of the CPU the test runs on and moves by
some 20 % between CPUs).  Per-token impacts of the 1232-token batch, fp32: relative error
median 6.5e-7, max 3.4e-4 (on an impact of 1.8e-4: |err| 6e-8), max |err| 3.2e-7.

No route showed a device bug.  What two wrong kernels do to these tests is written at
test_batch_invariance_many_docs."""
import functools
import os

import numpy as np
import pytest

import encoder_cases as C
import pairwise_cases as P

pytestmark = pytest.mark.gpu

R = P.ROUTE_CASES
CASE_PRECS = [(n, p) for n in R for p in P.ROUTE_PRECS[n]]


@functools.lru_cache(maxsize=None)
def E():
    from improving_learned_index_amd import _lib
    from improving_learned_index_amd import encoder

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible (GPU test run without a GPU)")
    return encoder


def make_encoder(case, prec):
    cfg, sd, *_ = P.inputs(case)
    old = os.environ.pop("DI_NO_LN_FOLD", None)
    if prec.endswith("-nofold"):
        os.environ["DI_NO_LN_FOLD"] = "1"
    try:
        enc = E().DeviceEncoder(sd, P.device_config(E(), cfg, case.variant),
                                precision=prec.split("-")[0])
        assert enc.precision == prec.split("-")[0]  # (no shape that falls back to fp32)
        return enc
    finally:
        os.environ.pop("DI_NO_LN_FOLD", None)
        if old is not None:
            os.environ["DI_NO_LN_FOLD"] = old


@functools.lru_cache(maxsize=None)
def encoder(name, prec):
    return make_encoder(R[name], prec)


def packed(case):
    _, _, pad, mask, tt, ct = P.inputs(case)
    return C.pack(pad, mask) + (tt, ct)


@functools.lru_cache(maxsize=None)
def device_result(name, prec):
    """(single, pair, cu_pairs, attn) of a case through host arrays, once per precision."""
    out = encoder(name, prec).encode_pairwise(*packed(R[name]), attentions=True)
    for a in out:
        a.setflags(write=False)
    return out


def check_attn(got, want):
    rel = np.abs(got - want) / np.abs(want)
    print(f"attn relative error: median {np.median(rel):.3g} max {rel.max():.3g}")
    np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-6)


def check_scores(got, want_pre, want, atol):
    err = np.abs(got - want)
    print(f"pair scores: atol {atol:.3g}; max |err| {err.max():.3g}; "
          f"max (|err| - 1e-3 want) {(err - 1e-3 * want).max():.3g}; "
          f"positive on the device {np.mean(got > 0):.3f}")
    assert (err <= 1e-3 * want + atol).all(), float((err - 1e-3 * want).max())
    sure_zero = want_pre < -atol
    assert sure_zero.any() and (got[sure_zero] == 0).all()


def check_against_oracle(name, prec, out):
    single, pair, cu_pairs, attn = out
    _, wattn, pre, want = P.oracle(R[name])["full"]
    assert len(pair) == len(attn) == len(want) == cu_pairs[-1]
    check_attn(attn, wattn)
    check_scores(pair, pre, want, P.pair_atol(prec.split("-")[0], R[name]))


@pytest.mark.parametrize("name,prec", CASE_PRECS)
def test_route_against_float64(name, prec):
    """One run per case and precision of pairwise_cases.ROUTE_PRECS; the measured errors
    are in the module docstring."""
    out = device_result(name, prec)
    check_against_oracle(name, prec, out)
    enc = encoder(name, prec)
    ids, cu, tt, ct = packed(R[name])
    assert out[0].tobytes() == enc.encode_packed(ids, cu, tt, ct).tobytes()


def _alone(name, prec, d):
    """Document d of a case encoded alone against its slices of the whole batch."""
    _, _, pad, mask, tt, ct = P.inputs(R[name])
    single, pair, cu_pairs, attn = device_result(name, prec)
    ids, cu = C.pack(pad[d:d + 1], mask[d:d + 1])
    t = tt[ct[d]:ct[d + 1]]
    s1, p1, cp1, a1 = encoder(name, prec).encode_pairwise(
        ids, cu, t, np.array([0, len(t)], np.int32), attentions=True)
    assert len(p1) == cp1[-1] == len(t) * (len(t) - 1) // 2
    assert s1.tobytes() == single[ct[d]:ct[d + 1]].tobytes()
    assert p1.tobytes() == pair[cu_pairs[d]:cu_pairs[d + 1]].tobytes()
    assert a1.tobytes() == attn[cu_pairs[d]:cu_pairs[d + 1]].tobytes()
    return len(p1)


def test_batch_invariance_many_docs():
    """Documents of the first group of 8, of later groups, on both sides of the 256th and
    the last, alone: bit for bit their slices of the 300.

    Checked by hand that the route is seen: with pair_attn_kernel's document taken as
    ((j / n_tiles) % 2) * 8 + x (documents from the 17th on get no attention) this test
    and the many_docs / many_docs_x3 oracle tests fail; with pair_prep_kernel giving every
    document of a thread's run the run's first offset (cu_sq[d] = part[t]) this test and
    the many_docs oracle test fail and nothing else in the suite does."""
    docs = (0, 8, 9, 10, 11, 255, 256, 258, 259, 299)
    with_pairs = 0
    for d in docs:
        with_pairs += _alone("many_docs", "fp32", d) > 0
    assert with_pairs >= 4  # (10, 11, 258, 259 keep all of 17 and some of 33 tokens)


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_batch_invariance_wide(prec):
    assert _alone("wide", prec, 0) == 300 * 299 // 2


def _pair_counts(ct):
    T = np.diff(ct.astype(np.int64))
    return np.concatenate([[0], np.cumsum(T * (T - 1) // 2)]).astype(np.int64)


class _DeviceCall:
    """One encode_pairwise_device call on torch device tensors.  The output buffers start
    as ones; the pair buffers are `room` floats longer than the batch's pairs."""

    def __init__(self, ids, cu, tt, ct, cu_pairs=None, n_pairs=None, room=0):
        import torch

        true_pairs = int(_pair_counts(ct)[-1])
        cu_pairs = _pair_counts(ct) if cu_pairs is None else cu_pairs
        self.n_pairs = true_pairs if n_pairs is None else n_pairs
        assert self.n_pairs <= true_pairs + room  # (the device writes n_pairs slots)
        lens = np.diff(cu)
        self.sizes = len(lens), int(cu[-1]), int(lens.max()), len(tt)
        self.dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda()
                    for a in (ids, cu, tt, ct, cu_pairs)]
        self.single = torch.ones(max(1, len(tt)), dtype=torch.float32, device="cuda")
        self.pair = torch.ones(max(1, true_pairs + room), dtype=torch.float32, device="cuda")
        self.attn = torch.ones_like(self.pair)
        torch.cuda.synchronize()

    def run(self, enc, flags=0):
        from improving_learned_index_amd import _lib

        ids, cu, tt, ct, cp = self.dev
        n_docs, n_tokens, max_len, n_terms = self.sizes
        try:
            enc.encode_pairwise_device(ids, cu, n_docs, n_tokens, max_len, tt, ct, n_terms, cp,
                                       self.n_pairs, self.single, self.pair, self.attn,
                                       _lib.DI_F_DEVICE_PTRS | flags)
        finally:
            enc.sync()
        return tuple(t.cpu().numpy() for t in (self.single, self.pair, self.attn))


@pytest.mark.parametrize("name", ["many_docs_x3", "wide"])
def test_device_pointer_route_equals_host_route(name):
    """Device pointers in and out (Mx sized by the bound n_terms min(n_terms, max_len), the
    device-side checks the only ones), waited for by the call or by sync() after
    DI_F_ASYNC: the host route's bytes."""
    from improving_learned_index_amd import _lib

    enc = encoder(name, "bf16x3")
    single, pair, _, attn = device_result(name, "bf16x3")
    for flags in (0, _lib.DI_F_ASYNC):
        s, p, a = _DeviceCall(*packed(R[name])).run(enc, flags)
        assert s.tobytes() == single.tobytes()
        assert p.tobytes() == pair.tobytes()
        assert a.tobytes() == attn.tobytes()


def test_device_side_refusals():
    """What only pair_prep_kernel can refuse on the device-pointer route (error bits 4 and
    8): the call raises, every pair slot it was told of reads 0, and the encoder goes on
    returning the earlier bytes."""
    from improving_learned_index_amd import _lib

    name = "many_docs_x3"
    enc = encoder(name, "bf16x3")
    ids, cu, tt, ct = packed(R[name])
    good = device_result(name, "bf16x3")
    T, cp = np.diff(ct.astype(np.int64)), _pair_counts(ct)
    n_pairs = int(cp[-1])
    d = 8 + int(np.argmax(T[8:] >= 2))  # a document of the second group of 8 with pairs
    assert d >= 8 and T[d] >= 2
    bad_tt = tt.copy()
    bad_tt[ct[d]], bad_tt[ct[d] + 1] = tt[ct[d] + 1], tt[ct[d]]
    bad_cp = cp.copy()
    bad_cp[d + 1:] += 1  # document d alone holds one pair too many
    for word, call in (("ascending", _DeviceCall(ids, cu, bad_tt, ct, room=1)),
                       ("cu_pairs", _DeviceCall(ids, cu, tt, ct, bad_cp, n_pairs + 1, room=1)),
                       ("cu_pairs", _DeviceCall(ids, cu, tt, ct, n_pairs=n_pairs - 1, room=1))):
        with pytest.raises(_lib.DIError) as e:
            call.run(enc)
        assert e.value.code == -1 and word in str(e.value), str(e.value)
        for buf in (call.pair, call.attn):
            got = buf.cpu().numpy()
            assert (got[:call.n_pairs] == 0).all() and (got[call.n_pairs:] == 1).all()
        s, p, _, a = enc.encode_pairwise(ids, cu, tt, ct, attentions=True)
        assert s.tobytes() == good[0].tobytes() and p.tobytes() == good[1].tobytes()
        assert a.tobytes() == good[3].tobytes()


def test_workspace_grows_and_is_used_small_again():
    """One encoder: a small batch, the wide one (Mx, uv, cu_sq and every row buffer grow),
    the small one again."""
    small = P.Case(1024, 1280, (130, 40), terms=P.all_terms((130, 40)))
    enc = make_encoder(R["wide"], "bf16x3")
    try:
        first = enc.encode_pairwise(*packed(small), attentions=True)
        assert len(first[1]) == 130 * 129 // 2 + 40 * 39 // 2 and (first[1] > 0).any()
        middle = enc.encode_pairwise(*packed(R["wide"]), attentions=True)
        third = enc.encode_pairwise(*packed(small), attentions=True)
    finally:
        enc.close()
    for a, b in zip(first, third):
        assert a.tobytes() == b.tobytes()
    check_against_oracle("wide", "bf16x3", middle)
    for a, b in zip(middle, device_result("wide", "bf16x3")):
        assert a.tobytes() == b.tobytes()


def test_long_token_impacts_against_float64():
    """The fp32 encoder's first run above 512 tokens: every token's impact of the (1232,
    17) batch against the float64 oracle, the project's fp32 bound."""
    c = R["long"]
    cfg, sd, pad, mask, *_ = P.inputs(c)
    ids, cu, _, _ = packed(c)
    got = encoder("long", "fp32").encode_packed(ids, cu, token_impacts=True)
    want = C.oracle(sd, cfg, pad, mask, act="relu")
    assert len(got) == len(want) == 1249 and 0.2 < np.mean(want > 0) < 0.8
    pos = want > 0
    rel = np.abs(got[pos] - want[pos]) / want[pos]
    print(f"token impacts: relative error median {np.median(rel):.3g} max {rel.max():.3g}; "
          f"max |err| {np.abs(got - want).max():.3g}")
    C.assert_fp32_bound(got, want)


def test_long_one_token_more_is_refused():
    """1233 tokens exceed the LDS panel: DI_ERANGE before any launch, and the encoder then
    returns the 1232 result."""
    from improving_learned_index_amd import _lib

    c = R["long"]
    enc = encoder("long", "fp32")
    good = device_result("long", "fp32")
    pad, mask = C.batch(np.random.default_rng(1), [1233, 17], 1024)
    ids, cu = C.pack(pad, mask)
    _, _, tt, ct = packed(c)
    with pytest.raises(_lib.DIError) as e:
        enc.encode_pairwise(ids, cu, tt, ct)
    assert e.value.code == -4 and "1233" in str(e.value)
    again = enc.encode_pairwise(*packed(c), attentions=True)
    for a, b in zip(again, good):
        assert a.tobytes() == b.tobytes()
